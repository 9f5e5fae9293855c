// K4: BM25 over CSR postings. Replaces BM25Okapi(tokenized_corpus).get_scores(tokenized_query) and the /max
// normalisation of /root/reference/rag/retrieval.py:324-347 (rank-bm25 0.2.2 semantics, float64).
//
// Integer/gather work, not a GEMM (89 % of the posting reads hit L2: frequent terms are shared by the batch's queries):
//   load   : per-posting impact w = idf * tf*(k1+1) / (tf + k1*(1 - b + b*dl/avgdl)) precomputed once in float64 with
//            rank-bm25's operation order -> postings are (doc int32, w float64): 12 B each, no doc_len gather, no multiply
//            later. A per-term BRACKET table (first posting at every 2^shift-th document, built once on the GPU) replaces
//            the two 20-step dependent binary searches per (block, token) that dominated the first version (36 ms/batch).
//            The table is two-level in the vocabulary: a term's bracket width is the smallest power of two >= the
//            2048-document range for which the table stays under df/4 entries, so long posting lists get the direct
//            per-range row (zero search steps, as before), the middle of the distribution coarser rows (a 1-3 step
//            search inside one bracket), and terms with fewer than 8 postings no row at all (a <= 3 step search of the
//            whole list). Table bytes <= nnz bytes = 1/12 of the postings for ANY vocabulary (r2's dense
//            V x n_ranges table was 122 GB for 5M terms on a 12.5M-document shard).
//   score  : one 256-thread workgroup per (query, 2048-doc range). The range's float64 accumulators live in LDS (20.5 KiB
//            with the scratch: SEVEN workgroups per CU, so one's posting round trips and token barriers hide behind the
//            others' adds; hybrid batch of 1024 on one box: 16384 docs x 1024 threads = one workgroup per CU 132.8 k q/s,
//            8192 x 1024 138.2 k, 4096 x 512 144.8 k, 2048 x 256 151.2 k); for each query token IN ORDER the block adds the
//            term's impacts of this doc range (docs are unique inside one posting list -> one read-add-write per
//            accumulator per token, and per-document summation order is the query-token order, exactly as `score += ...`
//            in get_scores -> bit-identical float64). 4 consecutive postings per thread per trip, the next trip in flight
//            across the token barrier.
//            Algorithmic traffic per query = sum over tokens of df*12 B; accumulators never touch HBM.
//   select : STAGED. The first BM_FIRST_RANGES ranges get an exact per-range top-k (8-pass radix select on order-
//            preserving keys, ties -> lower doc id, i.e. Python's stable sort); bm25_tau_kernel takes the k-th best key
//            over them (a lower bound of the global k-th); every other range only compacts its keys >= tau (exact select
//            as the fallback when more than k survive). Then a per-query merge of the partial lists.
// The same machinery serves a second resident index, the LEARNED-SPARSE one (rag_sparse_*, end of this file): postings
// (doc int32, weight float32), a float32 weight per query token, score += (double)qw * (double)w, and a top-k that holds only
// documents with a score > 0 - posting form 2 of bm25_range_body.
#include "common.h"

#include <cmath>
#include <cstring>
#include <memory>

typedef int int4u __attribute__((ext_vector_type(4), aligned(4)));          // posting segments start at any posting
typedef double double2u __attribute__((ext_vector_type(2), aligned(8)));
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));
#ifndef BM_RANGE            // -DBM_RANGE / -DBM_THREADS: variant builds by tools/bm25_variant_build.sh
#define BM_RANGE 2048
#endif
#ifndef BM_THREADS
#define BM_THREADS 256
#endif
#define BM_SEG (BM_RANGE / BM_THREADS)      // 8 contiguous docs per thread
// accumulator i lives at LDS double i + i/32 (one pad double per 32 docs). The padding dates from 32 docs per thread, where it
// made the per-thread segment reads of the select conflict-free; with 8 docs per thread it still spreads the lanes (lane t
// starts at bank pair 8(t%4) + t/4: at most 2-way instead of 8-way). The adds of the token loop fall on random banks either way.
#define SC_IDX(i) ((i) + ((i) >> 5))
// the same place as an LDS byte offset, from an UNSIGNED index: shift, add-and-shift (the pointer form &sc[SC_IDX(i)] costs the
// token loop two more vector instructions per posting, and that loop is bound by vector-instruction issue - DESIGN 4.2)
#define SC_OFF(u) ((((uint32_t)(u)) + (((uint32_t)(u)) >> 5)) << 3)
#define BM_SC_DOUBLES (BM_RANGE + BM_RANGE / 32)
#define BM_LDS_BYTES (BM_SC_DOUBLES * 8 + 4096)

// everything a (workgroup, token) needs to know about the token's term: ONE 32-byte load
struct __attribute__((aligned(32))) bm_term_meta {
    int64_t post;       // first posting of the term (indptr[t])
    int64_t tab;        // first entry of the term's bracket table in range_tab
    double idf;
    int32_t df;         // number of postings
    int32_t shift;      // log2(documents per bracket); BM_NO_TAB: no table, the bracket is the whole list
};
#define BM_NO_TAB 63
#define BM_TAB_DIV 4    // a term's table may take df / 4 entries (4 B each): table bytes <= nnz bytes = 1/12 of the postings
#define BM_RANGE_LOG2 (31 - __builtin_clz(BM_RANGE))
static_assert((BM_RANGE & (BM_RANGE - 1)) == 0, "BM_RANGE must be a power of two");

struct rag_bm25_index {
    int64_t n_docs = 0, n_terms = 0, nnz = 0;
    dev_buf<int32_t> doc;
    dev_buf<double> w;
    // OPTIONAL compact form (option bm25_packed at load time): 4-byte postings (doc & (BM_RANGE - 1)) | code << BM_RANGE_LOG2, code =
    // tf rank * n_dl + length rank, and the table g[code] = tf (k1+1) / (tf + k1 (1 - b + b dl / avgdl)) shared by all terms
    // (impact = idf * g, the same float64 product): 8 B per posting resident instead of 12 (`doc` stays for the plan kernel's
    // searches, `w` is not built) and a third of the streamed bytes - but the scoring loop gets SLOWER (1M documents, 1024 queries:
    // 4.22 against 3.36 ms): four 8-byte table gathers per chunk cost the texture path more than the two coalesced impact loads
    // they replace. The default therefore streams (doc i32, impact f64).
    dev_buf<uint32_t> packed;
    dev_buf<double> gtab;
    int64_t n_codes = 0;
    // LEARNED-SPARSE form (rag_sparse_load_host; the index of rag_ctx::sparse): the posting's weight as the caller's float32, 8 B
    // per posting with `doc`; `w` is not built, every term's idf is 1 and the QUERY carries a float32 weight per token
    // (a device array of the call, bm_range_call::qweights). A tail is of the same form; no refresh, raw scores.
    dev_buf<float> wf;
    dev_buf<bm_term_meta> meta;        // [n_terms]
    dev_buf<int32_t> range_tab;        // concatenated per-term tables: entry c = first posting (rel. to meta.post) with doc >= c << shift
    int64_t tab_entries = 0;
    int n_ranges = 0;
    dev_buf<char> ws;                  // base: grow-only workspace of the device entry points, carved per call (bm25_ws_planes)
    double avgdl = 0, k1 = 1.5, b = 0.75;
    double neg_idf_absmax = 0;         // largest |idf| among the negative idf values (0: none), for bm25_negative_bound_args
    int normalize = 1;                 // 0: top-k scores stay raw (row-sharded search divides by the GLOBAL max after the merge)
    // ---- appendable postings (rag_bm25_append_host / rag_bm25_fold). The BASE is the index as loaded; ONE TAIL - an index of
    // the same layout, always in the (doc, impact) form - holds the postings of the rows [n_docs, n_docs + tail_docs) appended
    // since. The tail numbers its documents from the start of the base's last 2048-document range (row0 = n_docs rounded down to a
    // range), so its ranges are the index's own ranges and a row's accumulator sits where a merged index would put it; the
    // boundary range exists in both segments and `first` = n_docs - row0 keeps the tail from emitting the base's rows.
    // Both resident indexes of a handle - the BM25 postings and the learned-sparse postings - are appended, folded and compacted
    // through the same code (bm_slot); a learned-sparse tail carries float32 weights as its base does.
    std::unique_ptr<rag_bm25_index> tail;
    int64_t tail_docs = 0;             // base: documents the tail covers
    int64_t appends = 0, folds = 0;    // base: since the load
    std::vector<int64_t> indptr_h;     // host copy of the posting offsets [n_terms + 1] (per-term concatenation is planned on the host)
    std::vector<double> idf_h;         // base: frozen idf of every known term, loaded and appended (size = terms known so far)
    dev_buf<int64_t> indptr_d;         // tail: the offsets on the device (source of the next append / the fold)
    int64_t row0 = 0;                  // tail: index row of its local document 0
    int first = 0;                     // tail: local documents below this are the base's
    // ---- what a statistics refresh needs (option bm25_keep_tf at load time; rag_bm25_refresh). Each segment keeps the length
    // of its documents, an unpacked segment the term frequency of every posting beside `doc` / `w`, a packed base the two value
    // tables its impact table is built from. Every operation that moves postings (append, fold, compaction) moves these along.
    bool keep_tf = false;
    dev_buf<uint16_t> tf16;            // [nnz] parallel to doc / w (unpacked segments)
    dev_buf<int32_t> dl;               // [n_docs] length of local document d (a tail's entries below `first` are unused, 0)
    dev_buf<double> tfv, dlv;          // packed base: distinct term frequencies / document lengths (gtab = their product table)
    uint32_t n_dl = 0;                 // packed base: entries of dlv
};
static inline int64_t bm_total_docs(const rag_bm25_index* ix) { return ix->n_docs + ix->tail_docs; }
static inline int bm_total_ranges(const rag_bm25_index* ix) { return ix->n_ranges + (ix->tail ? ix->tail->n_ranges : 0); }

// q_freq * (k1 + 1) / (q_freq + k1 * (1 - b + b * doc_len / avgdl))   -- same association as rank-bm25. The ONE place this is
// written: the load, the packed table and the statistics refresh all call it, so their impacts agree bit for bit.
__device__ __forceinline__ double bm_tf_factor(double f, double dl, double avgdl, double k1, double b) {
    const double num = f * (k1 + 1.0);
    const double t1 = (b * dl) / avgdl;
    const double t2 = (1.0 - b) + t1;
    const double den = f + k1 * t2;
    return num / den;
}

// The file's launch idiom for "one thread per element, 256 per workgroup". The arguments are converted to the kernel's parameter
// types here (a dev_buf to its pointer, nullptr to a typed null).
template <class... P, class... A>
static inline void bm_launch_1d(void (*kernel)(P...), int64_t n, hipStream_t st, A&&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<P>(args)...);
}

// The owner search, written once: the last t in [0, n) with key(t) <= p, for non-decreasing keys with key(0) <= p. The keys are
// the starts of per-term stretches (postings, or bracket-table entries). THE EMPTY-LIST RULE: a term with an empty stretch shares
// its start with the next term, so among equal keys the LAST t is the owner of p - every caller relies on it.
template <class Key>
__device__ __forceinline__ int64_t bm_last_le(int64_t n, int64_t p, Key key) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (key(mid) <= p) lo = mid; else hi = mid;
    }
    return lo;
}
// term of posting p, from CSR offsets / from the segment's term metadata
struct bm_term_by_offsets {
    const int64_t* indptr; int64_t n_terms;
    __device__ __forceinline__ int64_t operator()(int64_t p) const { return bm_last_le(n_terms, p, [&](int64_t t) { return indptr[t]; }); }
};
struct bm_term_by_meta {
    const bm_term_meta* meta; int64_t n_terms;
    __device__ __forceinline__ int64_t operator()(int64_t p) const { return bm_last_le(n_terms, p, [&](int64_t t) { return meta[t].post; }); }
};

// The impact of every posting, one thread each: the load (int32 tf; the term found in the metadata it has just uploaded), an
// appended block (int32 tf, CSR offsets) and the statistics refresh (the kept uint16 tf, metadata) run this one kernel, so their
// products agree bit for bit. The impact is stored already multiplied by the term's idf: `idf * (...)` is the product rank-bm25
// adds to the score, so the scoring loop is a pure load + add (one float64 multiply and one LDS lookup fewer per posting).
template <class TF, class TermOf>
__global__ void bm25_impact_kernel(const TermOf term_of, const int32_t* __restrict__ doc, const TF* __restrict__ tf,
                                   const int32_t* __restrict__ doc_len, int64_t nnz, double avgdl, double k1, double b,
                                   const double* __restrict__ idf, double* __restrict__ w) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const double f = (double)tf[p];
    const double dl = (double)doc_len[doc[p]];
    w[p] = idf[term_of(p)] * bm_tf_factor(f, dl, avgdl, k1, b);
}

// packed postings (see rag_bm25_index): one thread per posting
__global__ void bm25_pack_kernel(const int32_t* __restrict__ doc, const int32_t* __restrict__ tf, const uint32_t* __restrict__ tf_rank,
                                 const uint32_t* __restrict__ dl_rank_of_doc, int64_t nnz, uint32_t n_dl, uint32_t* __restrict__ packed) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const int32_t d = doc[p];
    packed[p] = ((uint32_t)d & (BM_RANGE - 1)) | ((tf_rank[tf[p]] * n_dl + dl_rank_of_doc[d]) << BM_RANGE_LOG2);
}

// g[ti * n_dl + di] for the ti-th distinct term frequency and the di-th distinct document length - the second factor of
// rank-bm25's `idf * (q_freq * (k1 + 1) / (q_freq + k1 * (1 - b + b * doc_len / avgdl)))`, same association as bm25_impact_kernel
__global__ void bm25_gtab_kernel(const double* __restrict__ tf_values, const double* __restrict__ dl_values, int64_t n_codes, uint32_t n_dl,
                                 double avgdl, double k1, double b, double* __restrict__ gtab) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_codes) return;
    gtab[c] = bm_tf_factor(tf_values[c / n_dl], dl_values[c % n_dl], avgdl, k1, b);
}

__device__ __forceinline__ int64_t lower_bound_doc(const int32_t* __restrict__ doc, int64_t lo, int64_t hi, int target) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (doc[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Host-side plan of the bracket tables: shift and entry count per term (see the header comment). n_pad = documents rounded
// up to a whole range; a table with shift g has ceil(n_pad / 2^g) + 1 entries (the last one = df).
static inline int64_t bm_tab_entries(int64_t n_pad, int g) { return ((n_pad + ((int64_t)1 << g) - 1) >> g) + 1; }
static inline int bm_plan_term(int64_t df, int64_t n_pad, int64_t* entries_out) {
    const int64_t budget = df / BM_TAB_DIV;
    int g = BM_RANGE_LOG2;
    while (bm_tab_entries(n_pad, g) > budget && bm_tab_entries(n_pad, g) > 2) ++g;
    const int64_t e = bm_tab_entries(n_pad, g);
    if (e > budget || e <= 2) { *entries_out = 0; return BM_NO_TAB; }      // one bracket = the whole list: no table needed
    *entries_out = e;
    return g;
}

// one thread per table entry; its term is the owner (bm_last_le) among the tables' starts: a term without a table has an empty stretch
__global__ void bm25_range_table_kernel(const bm_term_meta* __restrict__ meta, const int32_t* __restrict__ doc, int64_t n_terms,
                                        int64_t n_entries, int32_t* __restrict__ range_tab) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const int64_t lo = bm_last_le(n_terms, i, [&](int64_t t) { return meta[t].tab; });
    const bm_term_meta m = meta[lo];
    const int64_t target = (i - m.tab) << m.shift;
    range_tab[i] = target > 0x7fffffff ? m.df : (int32_t)(lower_bound_doc(doc, m.post, m.post + m.df, (int)target) - m.post);
}

// lower bound of `tg` in the ascending doc list dl[lo, hi): binary steps while the bracket is longer than 8 postings, then ONE
// round trip: the (up to) 8 remaining doc ids come as two 16-byte loads and are counted (the arrays carry 8 postings of padding)
__device__ __forceinline__ int bm_search(const int32_t* __restrict__ dl, int lo, int hi, int64_t tg) {
    while (hi - lo > 8) {
        const int mid = (lo + hi) >> 1;
        if (dl[mid] < tg) lo = mid + 1; else hi = mid;
    }
    if (hi > lo) {
        const int4u v0 = *reinterpret_cast<const int4u*>(dl + lo), v1 = *reinterpret_cast<const int4u*>(dl + lo + 4);
        const int n = hi - lo;
        int c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c += (j < n) && (v0[j] < tg);
            c += (j + 4 < n) && (v1[j] < tg);
        }
        lo += c;
    }
    return lo;
}

// bracket [lo, hi] of the term's table that holds lower_bound(tg); a target ON a bracket edge is the entry itself (always the
// case for the direct per-range rows of long lists); no table: the whole list
__device__ __forceinline__ void bm_bracket(const bm_term_meta& m, const int32_t* __restrict__ range_tab, int64_t tg, int& lo, int& hi) {
    lo = 0;
    hi = m.df;
    if (m.shift != BM_NO_TAB) {
        const int32_t* tb = range_tab + m.tab;
        const int64_t c = tg >> m.shift;
        lo = tb[c];
        hi = (tg & (((int64_t)1 << m.shift) - 1)) ? tb[c + 1] : lo;
    }
}

// ---- per-call PLAN: the posting offsets of every (query token, doc range) ------------------------------------------------
// plan_off[q][slot][r] = first posting (relative to the term's list) with doc >= r * BM_RANGE, r = 0 .. n_ranges, for the first
// BM_PLAN_T tokens of query q; plan_meta[q][slot] = the term's first posting and idf (idf 0: unknown token). One thread per
// (query, range edge), looping over the query's tokens: bracket lookup + in-bracket search, all independent - the searches the
// two-level table needs run here, massively parallel, instead of at the head of every scoring workgroup's dependent chain.
// The scoring kernel then reads two adjacent plan entries per token, exactly as it read r2's dense per-term table.
// The plan holds plan_t <= BM_PLAN_T token slots per query, chosen per call so that the table stays under BM_PLAN_BUDGET bytes
// (64 slots x 6,104 ranges x 4 B = 1.56 MB per query on a 12.5M-document shard whatever the queries' real token counts,
// 1.6 GB at 1,024 queries); tokens past the plan are searched inside the scoring kernel, so results do not depend on plan_t.
#define BM_PLAN_T 64
#define BM_PLAN_BUDGET ((size_t)512 << 20)
struct __attribute__((aligned(16))) bm_plan_meta { int64_t post; double idf; };

// WEIGHTED (the learned-sparse index): the float64 slot carries the query token's weight instead of the term's idf - 0 for an
// unknown term and for a weight that is not > 0 (NaN included), which is what "adds nothing" means to the scoring kernel.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void bm25_plan_kernel(const bm_term_meta* __restrict__ meta, const int32_t* __restrict__ doc,
                                                         const int32_t* __restrict__ range_tab, int n_ranges, int64_t n_terms,
                                                         const int32_t* __restrict__ term_ptr, const int32_t* __restrict__ terms,
                                                         int32_t* __restrict__ plan_off, bm_plan_meta* __restrict__ plan_meta, int plan_t,
                                                         const float* __restrict__ qweights) {
    const int q = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    const int t0 = term_ptr[q], nt = min(plan_t, term_ptr[q + 1] - t0);
    const int64_t tg = (int64_t)r * BM_RANGE;
    for (int s = 0; s < nt; ++s) {
        const int t = terms[t0 + s];
        const bool ok = t >= 0 && t < n_terms;               // out-of-vocabulary token: idf.get(q) is None -> 0
        bm_term_meta m = {0, 0, 0.0, 0, BM_NO_TAB};
        if (ok) m = meta[t];
        if constexpr (WEIGHTED) {
            if (r == 0) {
                const float qw = qweights[t0 + s];
                plan_meta[(size_t)q * plan_t + s] = {m.post, ok && qw > 0.0f ? (double)qw : 0.0};
            }
        } else
        if (r == 0) plan_meta[(size_t)q * plan_t + s] = {m.post, ok ? m.idf : 0.0};
        if (r <= n_ranges) {
            int lo, hi;
            bm_bracket(m, range_tab, tg, lo, hi);
            plan_off[((size_t)q * plan_t + s) * (n_ranges + 1) + r] = bm_search(doc + m.post, lo, hi, tg);
        }
    }
}

// Launch geometry of the scoring kernel: a 1-D grid over (range of this launch, query). The hardware hands consecutive workgroup
// ids to the 8 XCDs in turn, each XCD has its own 4 MiB L2, and one range's postings are ~2 MB: with the queries of a column
// running side by side on one XCD, the posting segments the queries share (frequent terms: most of the bytes) are served by
// that L2. n_groups splits the queries of a range into several columns when a launch has few ranges (the opening stages), so
// that every XCD owns >= 16 columns or so and the XCDs finish together. Few queries (qgroup_len = 0): range-major, the ranges
// of one query spread over the chip. The id -> XCD rule is a performance assumption only; any placement gives the same result.
struct bm_grid { unsigned blocks; int nr_l, n_queries, n_groups, qgroup_len, plan_t; };
// mode 1 (all-document scores) can also hand the index-level linear fusion what it needs, in the same pass over the accumulators:
// a float32 copy of the raw scores [q][ld] (the emission operand of the fused dense search) and the per-query maximum over the
// tenant's documents as an orderable key (atomicMax: order-independent, so the result is the bits a sequential max gives).
struct bm_dense_extra { float* raw32; int64_t ld; unsigned long long* max_key; };
// where a segment's documents sit in the index: local document d of the launch is index row row0 + d, local documents below
// `first` (range 0 only) belong to the other segment and are neither emitted nor written, out_ld = row length of the
// all-document score array (documents of BOTH segments). The base is {0, all documents, 0}.
struct bm_seg { int64_t row0; int64_t out_ld; int first; };
static bm_grid bm_make_grid(int nr_l, int Q, int linear) {
    bm_grid g{(unsigned)((int64_t)nr_l * Q), nr_l, Q, 1, 0, BM_PLAN_T};
    if (linear || Q < 128) return g;
    int G = 1;
    while (nr_l * G < 128 && G < 8 && Q / (2 * G) >= 64) G <<= 1;
    const int ql = (Q + G - 1) / G;
    const int64_t per_xcd = ((int64_t)nr_l * G + 7) / 8;
    g.blocks = (unsigned)(8 * per_xcd * ql);
    g.n_groups = G;
    g.qgroup_len = ql;
    return g;
}

// One workgroup per (query, doc range).
// mode 0: per-range top-k partials; mode 1: dense scores out[q][doc]
// PACKED (option bm25_packed, off by default - see rag_bm25_index): the scoring loop streams 4-byte postings (document number
// inside its 2048-document range | code of its (tf, doc length) pair) and looks the impact factor g(tf, dl) up in a table shared
// by all terms. Default: (doc i32, impact f64) = 12 bytes per posting.
// (SGPRs capped at 96: 256-thread workgroups are admitted 7 per CU up to 96 scalar registers, 6 from 97 on - MI355X_MICROARCH.md)
// The body of bm25_range_kernel below. qten: the tenant of every query of the launch (rag_*_tenants_*) or null - a compile-time null
// in the instantiations without QTEN, whose code is therefore what it was before queries had tenants of their own.
// FORM 0: (doc i32, impact f64); 1: PACKED; 2: SPARSE, the learned-sparse index - (doc i32, weight f32) postings, a float32 weight per
// query token (qweights; the planned tokens' weights come in the plan's float64 slot), score += (double)qw * (double)w, and a
// document whose score is not > 0 - one that matches nothing - is an EMPTY slot for the selection, like a hidden row.
template <int FORM>
__device__ __forceinline__ void bm25_range_body(const bm_term_meta* __restrict__ meta, const int32_t* __restrict__ doc,
                                                                 const double* __restrict__ w, const uint32_t* __restrict__ packed,
                                                                 const double* __restrict__ gtab,
                                                                 const int32_t* __restrict__ range_tab, int n_ranges,
                                                                 const int32_t* __restrict__ term_ptr, const int32_t* __restrict__ terms,
                                                                 int64_t n_docs, int64_t n_terms, int k, int mode,
                                                                 double* __restrict__ dense_out, uint64_t* __restrict__ part_key,
                                                                 uint32_t* __restrict__ part_row, int range_begin,
                                                                 const uint64_t* __restrict__ tau_key, int* __restrict__ part_cnt,
                                                                 const int32_t* __restrict__ tenants, int tenant_all,
                                                                 const int32_t* __restrict__ plan_off, const bm_plan_meta* __restrict__ plan_meta,
                                                                 const bm_grid gm, const bm_dense_extra dx, const bm_seg sg,
                                                                 const int32_t* __restrict__ qten, const float* __restrict__ wf,
                                                                 const float* __restrict__ qweights) {
    constexpr bool PACKED = FORM == 1, SPARSE = FORM == 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // workgroup -> (range, query), see bm_make_grid: XCD x (= workgroup id % 8) walks its columns (range, query group) one after the
    // other, every query of the group on the SAME range side by side, so a range's postings are fetched into that XCD's L2 once
    // per column instead of once per query that holds the term.
    int r, q;
    if (gm.qgroup_len == 0) {
        r = range_begin + (int)(blockIdx.x % (unsigned)gm.nr_l);
        q = (int)(blockIdx.x / (unsigned)gm.nr_l);
    } else {
        const unsigned x = blockIdx.x & 7u, s_ = blockIdx.x >> 3;
        const unsigned col = x + 8u * (s_ / (unsigned)gm.qgroup_len), qi = s_ % (unsigned)gm.qgroup_len;
        const int rl = (int)(col / (unsigned)gm.n_groups);
        q = (int)(col % (unsigned)gm.n_groups) * gm.qgroup_len + (int)qi;
        if (rl >= gm.nr_l || q >= gm.n_queries) return;
        r = range_begin + rl;
    }
    // the query's threshold (thresholded stages) is fetched up front: at the compaction step it would be an exposed global
    // round trip for every workgroup
    const uint64_t tk = tau_key != nullptr ? tau_key[q] : 0ull;
    // ... and so is the query's own tenant (rag_*_tenants_*; qten null: the launch's tenant for every query). Workgroup-uniform.
    const int tenant = tenant_of_query(qten, q, tenant_all);
    double* sc = reinterpret_cast<double*>(smem);                       // [BM_RANGE]
    int* hist = reinterpret_cast<int*>(smem + BM_SC_DOUBLES * 8);       // [256]
    int* wsum = hist + 256;                                             // [16] scratch
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)r * BM_RANGE;
    const int lim = (int)min((int64_t)BM_RANGE, n_docs - base);
    const int first = r == 0 ? sg.first : 0;                           // (scalar) first document of the range this segment owns
    const int64_t row_base = sg.row0 + base;                           // index row of the range's document 0
    // per-token metadata (idf, posting sub-range of this doc range) is fetched for up to 64 tokens IN PARALLEL into
    // LDS first: fetched inside the token loop it was ~4 dependent global round trips per token per block. The first batch's
    // loads (the planned tokens: two adjacent plan entries each) are issued BEFORE the accumulators are cleared, so that the
    // clearing runs under their round trip, and one barrier covers both.
    double* m_idf = reinterpret_cast<double*>(wsum + 16);              // [64]
    int64_t* m_a = reinterpret_cast<int64_t*>(m_idf + 64);             // [64]
    int* m_n = reinterpret_cast<int*>(m_a + 64);                       // [64]
    const int t0 = term_ptr[q], t1 = term_ptr[q + 1];
    double f_first = 0.0;
    int64_t a_first = 0;
    int n_first = 0;
    if (tid < min(gm.plan_t, t1 - t0)) {
        const bm_plan_meta pm = plan_meta[(size_t)q * gm.plan_t + tid];
        const int32_t* po = plan_off + ((size_t)q * gm.plan_t + tid) * (n_ranges + 1) + r;
        const int o0 = po[0], o1 = po[1];
        f_first = pm.idf;
        a_first = pm.post + o0;
        n_first = o1 - o0;
    }
    for (int i = tid; i < BM_SC_DOUBLES; i += BM_THREADS) sc[i] = 0.0;
    if (t1 <= t0) __syncthreads();                           // no token at all: the select below still needs the cleared array
    for (int tb = t0; tb < t1; tb += 64) {
        const int nb = min(64, t1 - tb);
        if (tid < nb) {
            double f = 0.0;
            int64_t a = 0;
            int n = 0;
            if (tb == t0 && tid < gm.plan_t) {               // planned tokens (at most one batch)
                f = f_first;
                a = a_first;
                n = n_first;
            } else {                                         // tokens past the plan (more than plan_t tokens in the query): search here
                const int t = terms[tb + tid];
                if (t >= 0 && t < n_terms) {
                    const bm_term_meta m = meta[t];
                    int lo0, hi0, lo1, hi1;
                    bm_bracket(m, range_tab, base, lo0, hi0);
                    bm_bracket(m, range_tab, base + BM_RANGE, lo1, hi1);
                    const int s0 = bm_search(doc + m.post, lo0, hi0, base);
                    const int e0 = bm_search(doc + m.post, max(lo1, s0), hi1, base + BM_RANGE);
                    f = m.idf;
                    if constexpr (SPARSE) {
                        const float qw = qweights[tb + tid];
                        f = qw > 0.0f ? (double)qw : 0.0;
                    }
                    a = m.post + s0;
                    n = e0 - s0;
                }
            }
            m_idf[tid] = f;
            m_a[tid] = a;
            m_n[tid] = f == 0.0 ? 0 : n;                     // (idf or 0) * x == 0: adds nothing
        }
        __syncthreads();
        // Docs are unique inside one posting list: exactly one add per accumulator per token, so a plain LDS read-add-write
        // is race-free inside a token (a no-return ds_add_f64 gives the same bits and was 2 % slower on the hybrid batch:
        // the float64 LDS atomic runs well below the rate of a b64 read + write); tokens are separated by a barrier so that
        // the per-document summation order is the token order (bit-identical to numpy). A (token, range) segment is only a few
        // postings per thread, so the loop is bound by one global round trip per token unless the NEXT chunk (4
        // consecutive postings per thread = 4 x BM_THREADS per block, possibly of the next token) is already in flight while the
        // current one is added: two register sets ping-pong, loads are unconditional (the arrays carry 4 postings of
        // padding) so the compiler keeps counted vmcnt waits, and the token barrier is a raw s_barrier behind
        // lgkmcnt(0) — __syncthreads would drain vmcnt and the prefetch with it.
        // The walk over (token, chunk) is the same in every thread. Each wave keeps the batch's token metadata in one VGPR
        // set (lane t = token t) and reads it with v_readlane at a scalar index: the three dependent LDS round trips per trip
        // (segment length for the step, base + length for the address, length for the tail test) become scalar moves.
        const int my_n = m_n[lane];
        const int64_t my_a = m_a[lane];
        const int my_a_lo = (int)(uint32_t)my_a, my_a_hi = (int)(my_a >> 32);
#define TOK_N(TI) __builtin_amdgcn_readlane(my_n, TI)
#define TOK_A(TI) (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(my_a_hi, TI) << 32) | (uint32_t)__builtin_amdgcn_readlane(my_a_lo, TI))
        int ti = 0, c = 0;
        while (ti < nb && TOK_N(ti) == 0) ++ti;
#define BM_NEXT(TI, C, NTI, NC)                                                                    \
            NTI = TI; NC = C + 1;                                                                  \
            if (NC * 4 * BM_THREADS >= TOK_N(TI)) {                                                \
                NC = 0;                                                                            \
                ++NTI;                                                                             \
                while (NTI < nb && TOK_N(NTI) == 0) ++NTI;                                         \
            }
#define BM_TOKEN_BARRIER asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
        if constexpr (PACKED) {
            // 4-byte postings: u = (doc - base) | code << 11; the impact is idf(token) * gtab[code], one float64 multiply - the same
            // product the 12-byte form stored (`idf * (num / den)`, rank-bm25's association), so the sums are bit-identical.
            // Three chunks are in flight per thread: the postings of chunk i + 2, the table values of chunk i + 1 (they need that
            // chunk's postings), the adds of chunk i.
            const double my_f = m_idf[lane];
            const int my_f_lo = (int)(uint32_t)__builtin_bit_cast(uint64_t, my_f), my_f_hi = (int)(__builtin_bit_cast(uint64_t, my_f) >> 32);
#define TOK_IDF(TI) __builtin_bit_cast(double, ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(my_f_hi, TI) << 32) | (uint32_t)__builtin_amdgcn_readlane(my_f_lo, TI))
#define BMP_LOAD(TI, C, U)                                                                         \
            {                                                                                      \
                const int64_t o_ = TOK_A(TI) + min((C) * 4 * BM_THREADS + tid * 4, max(TOK_N(TI) - 1, 0)); \
                U = *reinterpret_cast<const int4u*>(packed + o_);                                  \
            }
#define BMP_GATHER(U, G)                                                                           \
            {                                                                                      \
                G[0] = gtab[(uint32_t)U[0] >> BM_RANGE_LOG2]; G[1] = gtab[(uint32_t)U[1] >> BM_RANGE_LOG2]; \
                G[2] = gtab[(uint32_t)U[2] >> BM_RANGE_LOG2]; G[3] = gtab[(uint32_t)U[3] >> BM_RANGE_LOG2]; \
            }
#define BMP_ADD(TI, C, U, G)                                                                       \
            {                                                                                      \
                const int p_ = (C) * 4 * BM_THREADS + tid * 4, n_ = TOK_N(TI);                     \
                if (p_ < n_) {                                                                     \
                    const double f_ = TOK_IDF(TI);                                                 \
                    double* a0_ = &sc[SC_IDX(U[0] & (BM_RANGE - 1))];                              \
                    double* a1_ = p_ + 1 < n_ ? &sc[SC_IDX(U[1] & (BM_RANGE - 1))] : &sc[BM_SC_DOUBLES - 1]; \
                    double* a2_ = p_ + 2 < n_ ? &sc[SC_IDX(U[2] & (BM_RANGE - 1))] : &sc[BM_SC_DOUBLES - 2]; \
                    double* a3_ = p_ + 3 < n_ ? &sc[SC_IDX(U[3] & (BM_RANGE - 1))] : &sc[BM_SC_DOUBLES - 3]; \
                    const double v0_ = *a0_, v1_ = *a1_, v2_ = *a2_, v3_ = *a3_;                   \
                    *a0_ = v0_ + f_ * G[0];                                                        \
                    if (p_ + 1 < n_) *a1_ = v1_ + f_ * G[1];                                       \
                    if (p_ + 2 < n_) *a2_ = v2_ + f_ * G[2];                                       \
                    if (p_ + 3 < n_) *a3_ = v3_ + f_ * G[3];                                       \
                }                                                                                  \
            }
            // one turn of the pipeline: chunk X is added, chunk Y (postings in flight) gets its table values requested, the
            // postings of the chunk after Y are requested into Z. (tx, cx) / (ty, cy) walk the (token, chunk) sequence.
#define BMP_TURN(UX, GX, UY, GY, UZ)                                                               \
            {                                                                                      \
                int tz_ = ty, cz_ = cy;                                                            \
                bool more_z_ = false;                                                              \
                if (more_y) { BM_NEXT(ty, cy, tz_, cz_) more_z_ = tz_ < nb; }                      \
                { const int lt_ = more_z_ ? tz_ : ty, lc_ = more_z_ ? cz_ : cy; BMP_LOAD(lt_, lc_, UZ) } \
                BMP_GATHER(UY, GY)                                                                 \
                BMP_ADD(tx, cx, UX, GX)                                                            \
                if (!more_y) break;                                                                \
                if (ty != tx) BM_TOKEN_BARRIER;                                                    \
                tx = ty; cx = cy; more_y = more_z_;                                                \
                if (more_z_) { ty = tz_; cy = cz_; }        /* else (ty, cy) stays a valid (token, chunk) for the spare loads */ \
            }
            if (ti < nb) {
                int4u ua, ub, uc;
                double ga[4], gb[4], gc[4];
                int tx = ti, cx = c, ty = ti, cy = c;
                BMP_LOAD(tx, cx, ua)
                BM_NEXT(tx, cx, ty, cy)
                bool more_y = ty < nb;
                { const int lt_ = more_y ? ty : tx, lc_ = more_y ? cy : cx; BMP_LOAD(lt_, lc_, ub) }
                if (!more_y) { ty = tx; cy = cx; }
                BMP_GATHER(ua, ga)
                for (;;) {
                    BMP_TURN(ua, ga, ub, gb, uc)
                    BMP_TURN(ub, gb, uc, gc, ua)
                    BMP_TURN(uc, gc, ua, ga, ub)
                }
            }
#undef BMP_LOAD
#undef BMP_GATHER
#undef BMP_ADD
#undef BMP_TURN
#undef TOK_IDF
        } else
        if constexpr (SPARSE) {
            // (doc i32, weight f32): one 16-byte load from each plane per 4 postings, two register sets as in the unpacked loop
            // below; the weight becomes float64 and is multiplied by the token's float64 query weight (workgroup-uniform, read
            // with v_readlane). A float32 x float32 product is exact in float64: the only rounding is the add.
            const double my_f = m_idf[lane];
            const int my_f_lo = (int)(uint32_t)__builtin_bit_cast(uint64_t, my_f), my_f_hi = (int)(__builtin_bit_cast(uint64_t, my_f) >> 32);
#define TOK_QW(TI) __builtin_bit_cast(double, ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(my_f_hi, TI) << 32) | (uint32_t)__builtin_amdgcn_readlane(my_f_lo, TI))
#define SP_LOAD(TI, C, D, W)                                                                       \
            {                                                                                      \
                const int64_t o_ = TOK_A(TI) + min((C) * 4 * BM_THREADS + tid * 4, max(TOK_N(TI) - 1, 0)); \
                D = *reinterpret_cast<const int4u*>(doc + o_);                                     \
                W = *reinterpret_cast<const float4u*>(wf + o_);                                    \
            }
#define SP_ADD(TI, C, D, W)                                                                        \
            {                                                                                      \
                const int p_ = (C) * 4 * BM_THREADS + tid * 4, n_ = TOK_N(TI);                     \
                const double f_ = TOK_QW(TI);                                                      \
                char* const sb_ = reinterpret_cast<char*>(sc);                                     \
                if (((C) + 1) * 4 * BM_THREADS <= n_) {      /* a full chunk (uniform): no tail tests */ \
                    double* a0_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[0] - (int)base));       \
                    double* a1_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[1] - (int)base));       \
                    double* a2_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[2] - (int)base));       \
                    double* a3_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[3] - (int)base));       \
                    const double v0_ = *a0_, v1_ = *a1_, v2_ = *a2_, v3_ = *a3_;                   \
                    *a0_ = v0_ + f_ * (double)W[0];                                                \
                    *a1_ = v1_ + f_ * (double)W[1];                                                \
                    *a2_ = v2_ + f_ * (double)W[2];                                                \
                    *a3_ = v3_ + f_ * (double)W[3];                                                \
                } else if (p_ < n_) {                                                              \
                    double* a0_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[0] - (int)base));       \
                    double* a1_ = p_ + 1 < n_ ? reinterpret_cast<double*>(sb_ + SC_OFF(D[1] - (int)base)) : &sc[BM_SC_DOUBLES - 1]; \
                    double* a2_ = p_ + 2 < n_ ? reinterpret_cast<double*>(sb_ + SC_OFF(D[2] - (int)base)) : &sc[BM_SC_DOUBLES - 2]; \
                    double* a3_ = p_ + 3 < n_ ? reinterpret_cast<double*>(sb_ + SC_OFF(D[3] - (int)base)) : &sc[BM_SC_DOUBLES - 3]; \
                    const double v0_ = *a0_, v1_ = *a1_, v2_ = *a2_, v3_ = *a3_;                   \
                    *a0_ = v0_ + f_ * (double)W[0];                                                \
                    if (p_ + 1 < n_) *a1_ = v1_ + f_ * (double)W[1];                               \
                    if (p_ + 2 < n_) *a2_ = v2_ + f_ * (double)W[2];                               \
                    if (p_ + 3 < n_) *a3_ = v3_ + f_ * (double)W[3];                               \
                }                                                                                  \
            }
            if (ti < nb) {
                int4u da, db;
                float4u wa, wb;
                SP_LOAD(ti, c, da, wa)
                for (;;) {
                    int nti, nc;
                    BM_NEXT(ti, c, nti, nc)
                    const bool more1 = nti < nb;
                    { const int lt = more1 ? nti : ti, lc = more1 ? nc : c; SP_LOAD(lt, lc, db, wb) }
                    SP_ADD(ti, c, da, wa)
                    if (nti != ti) BM_TOKEN_BARRIER;
                    if (!more1) break;
                    ti = nti; c = nc;
                    BM_NEXT(ti, c, nti, nc)
                    const bool more2 = nti < nb;
                    { const int lt = more2 ? nti : ti, lc = more2 ? nc : c; SP_LOAD(lt, lc, da, wa) }
                    SP_ADD(ti, c, db, wb)
                    if (nti != ti) BM_TOKEN_BARRIER;
                    if (!more2) break;
                    ti = nti; c = nc;
                }
            }
#undef SP_LOAD
#undef SP_ADD
#undef TOK_QW
        } else
        if (ti < nb) {
            int4u da, db;
            double2u wa0, wa1, wb0, wb1;
#define BM_LOAD(TI, C, D, W0, W1)                                                                  \
            {                                                                                      \
                const int64_t o_ = TOK_A(TI) + min((C) * 4 * BM_THREADS + tid * 4, max(TOK_N(TI) - 1, 0)); \
                D = *reinterpret_cast<const int4u*>(doc + o_);                                     \
                W0 = *reinterpret_cast<const double2u*>(w + o_);                                   \
                W1 = *reinterpret_cast<const double2u*>(w + o_ + 2);                               \
            }
#define BM_ADD(TI, C, D, W0, W1)                                                                   \
            {                                                                                      \
                const int p_ = (C) * 4 * BM_THREADS + tid * 4, n_ = TOK_N(TI);                     \
                char* const sb_ = reinterpret_cast<char*>(sc);                                     \
                if (((C) + 1) * 4 * BM_THREADS <= n_) {      /* a full chunk (uniform): no tail tests */ \
                    double* a0_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[0] - (int)base));       \
                    double* a1_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[1] - (int)base));       \
                    double* a2_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[2] - (int)base));       \
                    double* a3_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[3] - (int)base));       \
                    const double v0_ = *a0_, v1_ = *a1_, v2_ = *a2_, v3_ = *a3_;                   \
                    *a0_ = v0_ + W0[0];                                                            \
                    *a1_ = v1_ + W0[1];                                                            \
                    *a2_ = v2_ + W1[0];                                                            \
                    *a3_ = v3_ + W1[1];                                                            \
                } else if (p_ < n_) {                                                              \
                    double* a0_ = reinterpret_cast<double*>(sb_ + SC_OFF(D[0] - (int)base));       \
                    double* a1_ = p_ + 1 < n_ ? reinterpret_cast<double*>(sb_ + SC_OFF(D[1] - (int)base)) : &sc[BM_SC_DOUBLES - 1]; \
                    double* a2_ = p_ + 2 < n_ ? reinterpret_cast<double*>(sb_ + SC_OFF(D[2] - (int)base)) : &sc[BM_SC_DOUBLES - 2]; \
                    double* a3_ = p_ + 3 < n_ ? reinterpret_cast<double*>(sb_ + SC_OFF(D[3] - (int)base)) : &sc[BM_SC_DOUBLES - 3]; \
                    const double v0_ = *a0_, v1_ = *a1_, v2_ = *a2_, v3_ = *a3_;                   \
                    *a0_ = v0_ + W0[0];                                                            \
                    if (p_ + 1 < n_) *a1_ = v1_ + W0[1];                                           \
                    if (p_ + 2 < n_) *a2_ = v2_ + W1[0];                                           \
                    if (p_ + 3 < n_) *a3_ = v3_ + W1[1];                                           \
                }                                                                                  \
            }
            BM_LOAD(ti, c, da, wa0, wa1)
            for (;;) {
                int nti, nc;
                BM_NEXT(ti, c, nti, nc)
                const bool more1 = nti < nb;
                { const int lt = more1 ? nti : ti, lc = more1 ? nc : c; BM_LOAD(lt, lc, db, wb0, wb1) }
                BM_ADD(ti, c, da, wa0, wa1)
                if (nti != ti) BM_TOKEN_BARRIER;
                if (!more1) break;
                ti = nti; c = nc;
                BM_NEXT(ti, c, nti, nc)
                const bool more2 = nti < nb;
                { const int lt = more2 ? nti : ti, lc = more2 ? nc : c; BM_LOAD(lt, lc, da, wa0, wa1) }
                BM_ADD(ti, c, db, wb0, wb1)
                if (nti != ti) BM_TOKEN_BARRIER;
                if (!more2) break;
                ti = nti; c = nc;
            }
#undef BM_LOAD
#undef BM_ADD
#undef BM_NEXT
#undef BM_TOKEN_BARRIER
#undef TOK_N
#undef TOK_A
        }
        __syncthreads();                                     // adds done before the next batch's metadata / the select
    }
    if (mode == 1) {
        double m = -INFINITY;
        for (int i = first + tid; i < lim; i += BM_THREADS) {
            // a deleted row scores 0.0 (it is not in the corpus the reference would score)
            const double v = row_visible(tenants, row_base + i, -1) ? sc[SC_IDX(i)] : 0.0;
            dense_out[(size_t)q * sg.out_ld + row_base + i] = v;
            if (dx.raw32 != nullptr) dx.raw32[(size_t)q * dx.ld + row_base + i] = (float)v;
            if (dx.max_key != nullptr && row_visible(tenants, row_base + i, tenant)) m = fmax(m, v);
        }
        if (dx.max_key != nullptr) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
            if (lane == 0 && m > -INFINITY) atomicMax(&dx.max_key[q], (unsigned long long)f64_orderable(m));
        }
        return;
    }
    // ---- exact top-k of sc[0..lim): radix select of the k-th largest key, ties by lower doc ------------
    const size_t po = ((size_t)q * n_ranges + r) * k;
    // part_cnt[q][r] = number of valid entries at the front of this (query, range) slot group; the merge only reads those
    // Tenant filter (`WHERE agent_id = %s`, rag/document_store.py:457): a document of another tenant is an EMPTY slot
    // (key 0, below every real score) from here on, so it can neither enter a partial list nor move the threshold.
    if (lim <= k) {
        for (int i = tid; i < k; i += BM_THREADS) {
            const bool mine = i < lim && i >= first && row_visible(tenants, row_base + i, tenant) && (!SPARSE || sc[SC_IDX(i)] > 0.0);
            part_key[po + i] = mine ? f64_orderable(sc[SC_IDX(i)]) : 0ull;
            part_row[po + i] = (uint32_t)(row_base + i);
        }
        if (tid == 0) part_cnt[(size_t)q * n_ranges + r] = lim;
        return;
    }
    const int seg0 = tid * BM_SEG;
    // this thread's BM_SEG docs, read once and UNCONDITIONALLY (the whole LDS array is initialised, a guarded read per doc was
    // eight serial LDS round trips); bit j of `valid` = doc seg0 + j exists and belongs to the tenant
    double sv[BM_SEG];
#pragma unroll
    for (int j = 0; j < BM_SEG; ++j) sv[j] = sc[SC_IDX(seg0 + j)];
    const int n_here = lim - seg0;
    unsigned valid = n_here >= BM_SEG ? (1u << BM_SEG) - 1u : (n_here <= 0 ? 0u : (1u << n_here) - 1u);
    if (first > seg0) valid &= first - seg0 >= BM_SEG ? 0u : ~((1u << (first - seg0)) - 1u);     // the other segment's documents: empty slots
    if (tenants != nullptr) {
#pragma unroll
        for (int j = 0; j < BM_SEG; ++j)
            if ((valid >> j & 1u) && !row_visible(tenants, row_base + seg0 + j, tenant)) valid &= ~(1u << j);
    }
    if constexpr (SPARSE) {                              // a document that matches nothing is never returned
#pragma unroll
        for (int j = 0; j < BM_SEG; ++j)
            if (!(sv[j] > 0.0)) valid &= ~(1u << j);
    }
    // Thresholded ranges (second stage, see bm25_launch_topk): tau_key[q] is the k-th best key over the first-stage
    // ranges, a lower bound of the global k-th. Only keys >= tau can reach the global top-k; a later range holds
    // about k * BM_RANGE / (docs of stage one) of them, so they are compacted in doc order (the merge sorts anyway) and the
    // 8-pass radix select — 26 us per block, three quarters of this kernel's time when run for every range — is
    // skipped. More than k survivors (possible, e.g. a tie plateau) falls through to the exact select below.
    // The test runs on the scores themselves: key(s) > tau_key <=> s > the double tau_key stands for (the key map is a monotone
    // bijection of the non-NaN doubles; an accumulator is never -0.0: it starts at +0.0 and x + y is -0.0 only for two -0.0),
    // one compare per document instead of a key conversion and two 64-bit compares; only survivors are converted.
    if (tau_key != nullptr) {
        const double tau_d = tk == 0ull ? -__builtin_inf() : f64_from_orderable(tk);
        unsigned pass = 0;
#pragma unroll
        // STRICTLY above tau: the running list already holds k documents with score >= tau, all of them from earlier ranges =
        // lower document numbers, and ties go to the lower document - a document that only EQUALS tau can never displace one of
        // them. (Scores of short queries tie in droves - same tf, same length -; with >= a plateau at tau passed whole, which is
        // what pushed the second stage into the exact per-range select and its merge to 1.4-2.8 k entries per query.)
        for (int j = 0; j < BM_SEG; ++j) pass |= (sv[j] > tau_d ? 1u : 0u) << j;
        pass &= valid;
        const int n_in = __builtin_popcount(pass);
        int sc_in = n_in;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(sc_in, o);
            if (lane >= o) sc_in += up;
        }
        if (lane == 63) hist[wv] = sc_in;
        __syncthreads();
        int off = sc_in - n_in, total_in = 0;
        for (int u = 0; u < BM_THREADS / 64; ++u) {
            if (u < wv) off += hist[u];
            total_in += hist[u];
        }
        if (total_in <= k) {
            if (pass) {
#pragma unroll
                for (int j = 0; j < BM_SEG; ++j)
                    if (pass >> j & 1u) {
                        part_key[po + off] = f64_orderable(sv[j]);
                        part_row[po + off] = (uint32_t)(row_base + seg0 + j);
                        ++off;
                    }
            }
            if (tid == 0) part_cnt[(size_t)q * n_ranges + r] = total_in;
            return;
        }
        __syncthreads();                                   // (uniform: total_in is the same in every thread) hist is reused by the select below
    }
    uint64_t keys[BM_SEG];
#pragma unroll
    for (int j = 0; j < BM_SEG; ++j) keys[j] = (valid >> j & 1u) ? f64_orderable(sv[j]) : 0ull;
    uint64_t prefix = 0ull;          // matched high bytes of the pivot
    int remaining = k;               // the pivot is the `remaining`-th largest among keys matching `prefix`
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        int cur = -1, run = 0;
#pragma unroll
        for (int j = 0; j < BM_SEG; ++j) {
            const int i = seg0 + j;
            const uint64_t key = keys[j];
            const bool match = i < lim && (pass == 0 || (key >> (shift + 8)) == prefix);
            if (!match) continue;
            const int d = (int)((key >> shift) & 0xFF);
            if (d == cur) { ++run; } else {
                if (run) atomicAdd(&hist[cur], run);
                cur = d; run = 1;
            }
        }
        if (run) atomicAdd(&hist[cur], run);
        __syncthreads();
        // suffix sums over the 256 bins (4 waves x 64 bins), find the bin holding the `remaining`-th largest
        int suf = 0;
        if (tid < 256) {
            int v = hist[tid];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_down(v, o);
                if (lane + o < 64) v += up;
            }
            suf = v;                                     // sum of bins [tid .. end of this wave's 64]
            if (lane == 0) wsum[wv] = v;
        }
        __syncthreads();
        if (tid < 256) {
            for (int u = wv + 1; u < 4; ++u) suf += wsum[u];      // bins of higher waves
            const int above = suf - hist[tid];                    // count of keys in bins > tid
            if (above < remaining && remaining <= suf) {          // exactly one bin satisfies this
                wsum[8] = tid;
                wsum[9] = remaining - above;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint64_t)wsum[8];
        remaining = wsum[9];
        __syncthreads();
    }
    const uint64_t pivot = prefix;                      // exact key of the k-th largest
    const int need_ties = remaining;                    // how many keys == pivot belong to the top-k (lowest docs first)
    // ordered collection: every key > pivot, plus the first `need_ties` keys == pivot in doc order
    int n_gt = 0, n_eq = 0;
#pragma unroll
    for (int j = 0; j < BM_SEG; ++j) {
        const bool in = (seg0 + j) < lim;
        n_gt += in && keys[j] > pivot;
        n_eq += in && keys[j] == pivot;
    }
    // block exclusive scans of n_gt and n_eq (thread order == doc order)
    int s_gt = n_gt, s_eq = n_eq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a1 = __shfl_up(s_gt, o), a2 = __shfl_up(s_eq, o);
        if (lane >= o) { s_gt += a1; s_eq += a2; }
    }
    if (lane == 63) { hist[wv] = s_gt; hist[16 + wv] = s_eq; }
    __syncthreads();
    int off_gt = s_gt - n_gt, off_eq = s_eq - n_eq, total_gt = 0;
    for (int u = 0; u < BM_THREADS / 64; ++u) {
        if (u < wv) { off_gt += hist[u]; off_eq += hist[16 + u]; }
        total_gt += hist[u];
    }
#pragma unroll
    for (int j = 0; j < BM_SEG; ++j) {
        const int i = seg0 + j;
        if (i >= lim) continue;
        const uint64_t key = keys[j];
        if (key > pivot) {
            part_key[po + off_gt] = key;
            part_row[po + off_gt] = (uint32_t)(row_base + i);
            ++off_gt;
        } else if (key == pivot) {
            if (off_eq < need_ties) {
                part_key[po + total_gt + off_eq] = key;
                part_row[po + total_gt + off_eq] = (uint32_t)(row_base + i);
            }
            ++off_eq;
        }
    }
    if (tid == 0) part_cnt[(size_t)q * n_ranges + r] = k;
}

// FORM: the posting form (bm25_range_body); QTEN: a tenant per query - the workgroup reads its query's, `tenant` is not read - instead
// of one tenant (or none) for the whole launch. The learned-sparse form (rag_sparse_*) reads float32 posting weights wf (`w`, `packed`,
// `gtab` are null) and a float32 weight per query token. A trailing parameter an instantiation does not use reaches the body as a
// compile-time null.
template <int FORM, bool QTEN>
__global__ __launch_bounds__(BM_THREADS) __attribute__((amdgpu_num_sgpr(96))) void bm25_range_kernel(
    const bm_term_meta* __restrict__ meta, const int32_t* __restrict__ doc, const double* __restrict__ w, const uint32_t* __restrict__ packed,
    const double* __restrict__ gtab, const int32_t* __restrict__ range_tab, int n_ranges, const int32_t* __restrict__ term_ptr,
    const int32_t* __restrict__ terms, int64_t n_docs, int64_t n_terms, int k, int mode, double* __restrict__ dense_out,
    uint64_t* __restrict__ part_key, uint32_t* __restrict__ part_row, int range_begin, const uint64_t* __restrict__ tau_key,
    int* __restrict__ part_cnt, const int32_t* __restrict__ tenants, int tenant, const int32_t* __restrict__ plan_off,
    const bm_plan_meta* __restrict__ plan_meta, const bm_grid gm, const bm_dense_extra dx, const bm_seg sg,
    const int32_t* __restrict__ qten, const float* __restrict__ wf, const float* __restrict__ qweights) {
    bm25_range_body<FORM>(meta, doc, w, packed, gtab, range_tab, n_ranges, term_ptr, terms, n_docs, n_terms, k, mode, dense_out, part_key,
                          part_row, range_begin, tau_key, part_cnt, tenants, tenant, plan_off, plan_meta, gm, dx, sg, QTEN ? qten : nullptr,
                          FORM == 2 ? wf : nullptr, FORM == 2 ? qweights : nullptr);
}

#define BM_MERGE 2048
__device__ __forceinline__ void bm_sort_pairs(uint64_t* k1, uint32_t* k2, int P, int tid, int nthreads) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += nthreads) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool first_block = ((i & k) == 0);
                    const bool a_before_b = k1[i] > k1[ixj] || (k1[i] == k1[ixj] && k2[i] < k2[ixj]);
                    if (first_block ? !a_before_b : a_before_b) {
                        const uint64_t t1 = k1[i]; k1[i] = k1[ixj]; k1[ixj] = t1;
                        const uint32_t t2 = k2[i]; k2[i] = k2[ixj]; k2[ixj] = t2;
                    }
                }
            }
            __syncthreads();
        }
    }
}

#define BM_FIRST_RANGES 4      // exact per-range top-k for these (8192 docs), thresholded compaction for the rest (2048-doc ranges: 2 -> 134.2 k hybrid q/s, 4 -> 151.2 k;
                               // 4096-doc ranges: 2 -> 144.8 k, 4 -> 143.3 k; 16384-doc ranges, BM25 leg alone: 1 -> 7.5 ms, 2 -> 4.87, 4 -> 5.08)
#ifndef BM_STAGE_GROWTH        // -DBM_STAGE_GROWTH: variant builds (tools/lib_ab.sh; r3: 4 -> 3.04 ms, 8 -> 2.88, 16 -> 3.05, 32 -> 3.44 per 1024-query batch)
#define BM_STAGE_GROWTH 8      // every thresholded stage covers up to 8x the ranges seen before it
#endif

// Folds the partial lists of the doc ranges [r_begin, r_end) into the query's RUNNING top-k (run_key / run_row [Q][k], key 0 =
// empty) and publishes tau_key[q] = its k-th key: a lower bound of the global k-th best, 0 ("everything passes") while fewer
// than k documents have been seen. One workgroup per query; windows of BM_MERGE - k new entries, bitonic sort in LDS.
// A thresholded range fills only the first part_cnt[q][r] of its k slots and the rest of the slot group holds whatever an
// earlier batch left there, so ONLY the counted fronts are read, for any number of ranges: they are walked in groups of 256
// (one prefix scan per group; a 12.5M-document shard has 763 ranges).
// last != 0: the running list is final -> ids / rows / scores (divided by max if > 0 else 1.0, rag/retrieval.py:343-345).
__global__ __launch_bounds__(256) void bm25_merge_stage_kernel(const uint64_t* __restrict__ part_key, const uint32_t* __restrict__ part_row,
                                                                const int* __restrict__ part_cnt, int n_ranges, int r_begin, int r_end,
                                                                int k, uint64_t* __restrict__ run_key, uint32_t* __restrict__ run_row,
                                                                int first, uint64_t* __restrict__ tau_key, int last,
                                                                const int64_t* __restrict__ idmap, int64_t id_base,
                                                                int64_t* __restrict__ ids_out, int32_t* __restrict__ rows_out,
                                                                double* __restrict__ scores_out, double* __restrict__ raw_max_out,
                                                                int normalize) {
    __shared__ uint64_t sk[BM_MERGE];
    __shared__ uint32_t sr[BM_MERGE];
    __shared__ int pre[257];                        // exclusive prefix of the entry counts of the current group of <= 256 ranges
    __shared__ int wtot[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint64_t* pk = part_key + (size_t)q * n_ranges * k;
    const uint32_t* pr = part_row + (size_t)q * n_ranges * k;
    for (int i = tid; i < BM_MERGE; i += 256) {
        const bool keep = !first && i < k;
        sk[i] = keep ? run_key[(size_t)q * k + i] : 0ull;
        sr[i] = keep ? run_row[(size_t)q * k + i] : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int r0 = r_begin; r0 < r_end; r0 += 256) {
        const int nr = min(256, r_end - r0);
        const int c = tid < nr ? min(part_cnt[(size_t)q * n_ranges + r0 + tid], k) : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if ((tid & 63) >= o) incl += up;
        }
        if ((tid & 63) == 63) wtot[tid >> 6] = incl;
        __syncthreads();
        int off = 0;
        for (int w = 0; w < (tid >> 6); ++w) off += wtot[w];
        pre[tid + 1] = off + incl;
        if (tid == 0) pre[0] = 0;
        __syncthreads();
        const int total = pre[nr];
        int pos = 0;
        while (pos < total) {
            // window = the smallest power of two that holds the running top-k plus what is left of this group (a stage usually
            // brings a few hundred entries: sorting 512 or 1024 slots instead of 2048 halves the merge time)
            int P = 256;
            while (P < BM_MERGE && P < k + (total - pos)) P <<= 1;
            const int room = P - k;
            const int take = min(room, total - pos);
            for (int i = tid; i < room; i += 256) {
                uint64_t key = 0ull;
                uint32_t row = 0xFFFFFFFFu;
                if (i < take) {                     // entry e -> range r with pre[r] <= e < pre[r+1] -> slot r*k + (e - pre[r])
                    const int e = pos + i;
                    int lo = 0, hi = nr;
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (pre[mid] <= e) lo = mid; else hi = mid;
                    }
                    const size_t slot = (size_t)(r0 + lo) * k + (e - pre[lo]);
                    key = pk[slot];
                    row = pr[slot];
                }
                sk[k + i] = key;
                sr[k + i] = row;
            }
            __syncthreads();
            bm_sort_pairs(sk, sr, P, tid, 256);
            pos += take;
        }
        __syncthreads();                            // every thread is done with pre[] / wtot[] before the next group's scan
    }
    for (int i = tid; i < k; i += 256) {
        run_key[(size_t)q * k + i] = sk[i];
        run_row[(size_t)q * k + i] = sr[i];
    }
    if (tid == 0 && tau_key != nullptr) tau_key[q] = sk[k - 1];        // 0 if fewer than k real keys so far
    if (!last) return;
    // top-1 raw score -> divisor (max if > 0 else 1.0), retrieval.py:344
    uint64_t u0 = sk[0];
    double mx = 1.0;
    if (u0 != 0ull) {
        const double top = f64_from_orderable(u0);
        if (top > 0.0) mx = top;
    }
    if (tid == 0 && raw_max_out) raw_max_out[q] = mx;
    for (int i = tid; i < k; i += 256) {
        const bool ok = sk[i] != 0ull;
        const double s = f64_from_orderable(sk[i]);
        ids_out[(size_t)q * k + i] = ok ? (idmap ? idmap[sr[i]] : id_base + (int64_t)sr[i]) : -1;
        if (rows_out) rows_out[(size_t)q * k + i] = ok ? (int32_t)sr[i] : -1;
        scores_out[(size_t)q * k + i] = ok ? (normalize ? s / mx : s) : 0.0;
    }
}

// ---- the same fold by SELECTION instead of sorting (k <= BMS_KMAX; the default) ----------------------------------------------
// The bitonic merge above sorts 512 .. 2048 slots per query and stage to keep 100 of them: 42 / 225 / 121 / 21 us for the four
// stages of a 1024-query batch at 1M documents, 0.41 of the 2.9 ms BM25 leg. Here ONE WAVE folds one query: the running list
// (sorted, k slots at the front of the wave's LDS window) and the stage's new entries (appended behind it, straight from the
// counted fronts of the partial lists) are loaded into registers, the k-th largest key is found bit by bit with ballots (64
// steps x one ballot per key register, no atomics, no sort - the dense path's select), ties at the k-th key are cut by the
// LOWEST ROWS with a second bitwise search over the rows of the tied entries, the k survivors are compacted and ranked by
// counting (k x k / 64 compares per lane). Result: the same list bit for bit (order: key descending, row ascending).
#define BMS_KMAX 256
#define BMS_CAP 2048                     // entries a wave selects from at once: k running + up to BMS_CAP - k new ones
#define BMS_WAVES 2
#define BMS_WAVE_BYTES (BMS_CAP * 12 + BMS_KMAX * 12)
#define BMS_LDS_BYTES (BMS_WAVES * BMS_WAVE_BYTES)
#define BMS_FENCE asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")       // one wave: LDS operations retire in order; this keeps the compiler honest

// top-k of wk/wr[0, total) -> wk/wr[0, k) sorted (key descending, row ascending), empty slots (0, 0xFFFFFFFF) behind
template <int NREG>
__device__ __forceinline__ void bms_select(uint64_t* __restrict__ wk, uint32_t* __restrict__ wr, uint64_t* __restrict__ tk,
                                           uint32_t* __restrict__ tr, int total, int k, int lane) {
    uint64_t key[NREG];
    uint32_t row[NREG];
#pragma unroll
    for (int e = 0; e < NREG; ++e) {
        const int i = e * 64 + lane;
        key[e] = i < total ? wk[i] : 0ull;
        row[e] = i < total ? wr[i] : 0xFFFFFFFFu;
    }
    BMS_FENCE;
    int n_valid = 0;
#pragma unroll
    for (int e = 0; e < NREG; ++e) n_valid += __popcll(__ballot(key[e] != 0ull));
    uint64_t pivot = 0ull;               // survivors: key > pivot, or key == pivot and ~row >= inv_pivot (0, 0: every real key)
    uint32_t inv_pivot = 0u;
    if (n_valid > k) {
        pivot = 0ull;
        int ge = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const uint64_t trial = pivot | (1ull << bit);
            int c = 0;
#pragma unroll
            for (int e = 0; e < NREG; ++e) c += __popcll(__ballot(key[e] >= trial));
            if (c >= k) { pivot = trial; ge = c; }
            if (c == k) break;
        }
        if (ge > k) {                    // a plateau at the k-th key: the m tied entries with the lowest rows stay
            int gt = 0;
#pragma unroll
            for (int e = 0; e < NREG; ++e) gt += __popcll(__ballot(key[e] > pivot));
            const int m = k - gt;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t trial = inv_pivot | (1u << bit);
                int c = 0;
#pragma unroll
                for (int e = 0; e < NREG; ++e) c += __popcll(__ballot(key[e] == pivot && ~row[e] >= trial));
                if (c >= m) inv_pivot = trial;
                if (c == m) break;
            }
        }
    }
    // compaction (any order) into the scratch list
    int n_s = 0;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int e = 0; e < NREG; ++e) {
        const bool in = key[e] != 0ull && (key[e] > pivot || (key[e] == pivot && ~row[e] >= inv_pivot));
        const uint64_t bt = __ballot(in);
        if (in) {
            const int d = n_s + __popcll(bt & lt_mask);
            tk[d] = key[e];
            tr[d] = row[e];
        }
        n_s += __popcll(bt);
    }
    BMS_FENCE;
    // rank by counting: slot of a survivor = the number of survivors that come before it
    for (int i = lane; i < k; i += 64) {
        wk[i] = 0ull;
        wr[i] = 0xFFFFFFFFu;
    }
    BMS_FENCE;
    for (int i = lane; i < n_s; i += 64) {
        const uint64_t a = tk[i];
        const uint32_t ar = tr[i];
        int rank = 0;
        for (int j = 0; j < n_s; ++j) {
            const uint64_t b = tk[j];
            rank += (b > a) || (b == a && tr[j] < ar);
        }
        wk[rank] = a;
        wr[rank] = ar;
    }
    BMS_FENCE;
}

__global__ __launch_bounds__(64 * BMS_WAVES) void bm25_merge_select_kernel(const uint64_t* __restrict__ part_key, const uint32_t* __restrict__ part_row,
                                                                         const int* __restrict__ part_cnt, int n_ranges, int r_begin, int r_end,
                                                                         int k, uint64_t* __restrict__ run_key, uint32_t* __restrict__ run_row,
                                                                         int first, uint64_t* __restrict__ tau_key, int last,
                                                                         const int64_t* __restrict__ idmap, int64_t id_base,
                                                                         int64_t* __restrict__ ids_out, int32_t* __restrict__ rows_out,
                                                                         double* __restrict__ scores_out, double* __restrict__ raw_max_out,
                                                                         int normalize, int n_queries) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = blockIdx.x * BMS_WAVES + wv;
    if (q >= n_queries) return;                              // whole wave; nothing below synchronises across waves
    uint64_t* wk = reinterpret_cast<uint64_t*>(smem + (size_t)wv * BMS_WAVE_BYTES);      // [BMS_CAP]
    uint64_t* tk = wk + BMS_CAP;                                                         // [BMS_KMAX]
    uint32_t* wr = reinterpret_cast<uint32_t*>(tk + BMS_KMAX);                           // [BMS_CAP]
    uint32_t* tr = wr + BMS_CAP;                                                         // [BMS_KMAX]
    const uint64_t* pk = part_key + (size_t)q * n_ranges * k;
    const uint32_t* pr = part_row + (size_t)q * n_ranges * k;
    for (int i = lane; i < k; i += 64) {
        wk[i] = first ? 0ull : run_key[(size_t)q * k + i];
        wr[i] = first ? 0xFFFFFFFFu : run_row[(size_t)q * k + i];
    }
    int n_win = 0;                                           // new entries behind the running list
#define BMS_FLUSH                                                                      \
    {                                                                                  \
        BMS_FENCE;                                                                     \
        const int tot_ = k + n_win;                                                    \
        if (tot_ <= 512) bms_select<8>(wk, wr, tk, tr, tot_, k, lane);                 \
        else if (tot_ <= 1024) bms_select<16>(wk, wr, tk, tr, tot_, k, lane);          \
        else bms_select<32>(wk, wr, tk, tr, tot_, k, lane);                            \
        n_win = 0;                                                                     \
    }
    for (int r0 = r_begin; r0 < r_end; r0 += 64) {
        const int nr = min(64, r_end - r0);
        const int c = lane < nr ? min(part_cnt[(size_t)q * n_ranges + r0 + lane], k) : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        int done = 0, base = 0;                              // ranges of this group already taken, and their entries
        while (done < nr) {
            const int room = BMS_CAP - k - n_win;
            const bool acc = lane >= done && lane < nr && incl - base <= room;
            const int n_acc = __popcll(__ballot(acc));       // a prefix of the remaining ranges (incl is monotone)
            if (n_acc > 0) {
                const int off = k + n_win + (incl - c - base);
                const bool small = acc && c <= 4;
                if (small) {
                    const size_t slot = (size_t)(r0 + lane) * k;
                    for (int j = 0; j < c; ++j) {
                        wk[off + j] = pk[slot + j];
                        wr[off + j] = pr[slot + j];
                    }
                }
                uint64_t big = __ballot(acc && c > 4);       // longer fronts (an exact range brings k entries): the whole wave copies
                while (big) {
                    const int L = __ffsll((unsigned long long)big) - 1;
                    big &= big - 1;
                    const int cL = __builtin_amdgcn_readlane(c, L), offL = __builtin_amdgcn_readlane(off, L);
                    const size_t slot = (size_t)(r0 + L) * k;
                    for (int j = lane; j < cL; j += 64) {
                        wk[offL + j] = pk[slot + j];
                        wr[offL + j] = pr[slot + j];
                    }
                }
                const int upto = __builtin_amdgcn_readlane(incl, done + n_acc - 1);
                n_win += upto - base;
                base = upto;
                done += n_acc;
            }
            if (done < nr) BMS_FLUSH                         // the window is full: fold, then go on with the rest of the group
        }
    }
    if (n_win > 0 || first) BMS_FLUSH
#undef BMS_FLUSH
    BMS_FENCE;
    for (int i = lane; i < k; i += 64) {
        run_key[(size_t)q * k + i] = wk[i];
        run_row[(size_t)q * k + i] = wr[i];
    }
    if (lane == 0 && tau_key != nullptr) tau_key[q] = wk[k - 1];      // 0 if fewer than k real keys so far
    if (!last) return;
    uint64_t u0 = wk[0];
    double mx = 1.0;
    if (u0 != 0ull) {
        const double top = f64_from_orderable(u0);
        if (top > 0.0) mx = top;
    }
    if (lane == 0 && raw_max_out) raw_max_out[q] = mx;
    for (int i = lane; i < k; i += 64) {
        const bool ok = wk[i] != 0ull;
        const double sc_ = f64_from_orderable(wk[i]);
        ids_out[(size_t)q * k + i] = ok ? (idmap ? idmap[wr[i]] : id_base + (int64_t)wr[i]) : -1;
        if (rows_out) rows_out[(size_t)q * k + i] = ok ? (int32_t)wr[i] : -1;
        scores_out[(size_t)q * k + i] = ok ? (normalize ? sc_ / mx : sc_) : 0.0;
    }
}

// per-call device buffers of a top-k search: partial lists [Q][n_ranges][k], counts [Q][n_ranges], running list, threshold
// + the per-call plan (see bm25_plan_kernel): plan.off [Q][plan_t][n_ranges + 1] int32, plan.meta [Q][BM_PLAN_T]
struct bm25_plan_ws { int32_t* off; bm_plan_meta* meta; };
struct bm25_topk_ws {
    uint64_t* part_key; uint32_t* part_row; int* part_cnt; uint64_t* run_key; uint32_t* run_row; uint64_t* tau;
    bm25_plan_ws plan;
};
struct bm25_topk_out {
    const int64_t* idmap; int64_t id_base; int64_t* ids; int32_t* rows; double* scores; double* raw_max; int normalize;
};

// Everything ONE scoring launch needs. An entry point fills the first row - what holds for the whole call: the index (seg = its
// base), the device query arrays with the learned-sparse index's float32 weight per token, k, the mode (0: per-range top-k partials;
// 1: all-document scores), the planned token slots per query (bm25_pick_plan_t, <= BM_PLAN_T) - and the tenants; the launch
// functions below fill the rest per segment and stage. An output that a launch does not write stays null.
struct bm_range_call {
    const rag_bm25_index* seg; const int32_t* term_ptr; const int32_t* terms; const float* qweights; int k, mode, plan_t;
    const int32_t* tenants = nullptr; int tenant = -1; const int32_t* qten = nullptr;      // per row (null: no filter) | the launch's | per query
    double* dense_out = nullptr; bm_dense_extra dx = {nullptr, 0, nullptr};                // mode 1: [Q][out_ld] + the linear fusion's extras
    int64_t out_ld = 0;                                                                    // documents of the whole index (both segments)
    uint64_t* part_key = nullptr; uint32_t* part_row = nullptr; int* part_cnt = nullptr;   // mode 0: the segment's partial lists and counts
    int range_begin = 0; const uint64_t* tau_key = nullptr;                                // first range of the launch; thresholded stage: tau
    bm25_plan_ws plan = {nullptr, nullptr};                                                // the segment's plan
};

// the scoring launch of nr_launch ranges from c.range_begin: the instantiation by the segment's posting form and by whether the
// queries carry tenants of their own
static void bm_launch_range(const rag_ctx* h, const bm_range_call& c, int nr_launch, int Q, hipStream_t st) {
    static constexpr decltype(&bm25_range_kernel<0, false>) kernels[3][2] = {{bm25_range_kernel<0, false>, bm25_range_kernel<0, true>},
                                                                             {bm25_range_kernel<1, false>, bm25_range_kernel<1, true>},
                                                                             {bm25_range_kernel<2, false>, bm25_range_kernel<2, true>}};
    const rag_bm25_index* s = c.seg;
    bm_grid gm = bm_make_grid(nr_launch, Q, h->opt.bm25_linear_grid);
    gm.plan_t = c.plan_t;
    const bm_seg sg = {s->row0, c.out_ld, s->first};
    launch(kernels[s->wf != nullptr ? 2 : s->packed != nullptr ? 1 : 0][c.qten != nullptr], dim3(gm.blocks), dim3(BM_THREADS), BM_LDS_BYTES,
           st, s->meta, s->doc, s->w, s->packed, s->gtab, s->range_tab, s->n_ranges, c.term_ptr, c.terms, s->n_docs, s->n_terms, c.k, c.mode,
           c.dense_out, c.part_key, c.part_row, c.range_begin, c.tau_key, c.part_cnt, c.tenants, c.tenant, c.plan.off, c.plan.meta, gm, c.dx,
           sg, c.qten, s->wf, c.qweights);
}

static int bm25_pick_plan_t(const rag_ctx* h, const rag_bm25_index* ix, int Q) {
    if (h->opt.bm25_plan_slots > 0) return std::min(BM_PLAN_T, h->opt.bm25_plan_slots);
    const size_t per_slot = (size_t)Q * (ix->n_ranges + 1 + (ix->tail ? ix->tail->n_ranges + 1 : 0)) * sizeof(int32_t);
    return (int)std::min<size_t>(BM_PLAN_T, std::max<size_t>(8, BM_PLAN_BUDGET / std::max<size_t>(1, per_slot)));
}
static size_t bm25_plan_off_total(const rag_bm25_index* ix, int Q, int plan_t) {
    return (size_t)Q * plan_t * (ix->n_ranges + 1 + (ix->tail ? ix->tail->n_ranges + 1 : 0));
}
static size_t bm25_plan_meta_total(const rag_bm25_index* ix, int Q) { return (size_t)Q * BM_PLAN_T * (ix->tail ? 2 : 1); }
// The segments of an index are walked base first. `call` as the entry point filled it, narrowed to segment sg of the index call.seg
// with its SLICE of the call's buffers w: the plan of the tail sits behind the base's in the same two buffers (offsets: all of the
// base's entries; metadata: Q x BM_PLAN_T), its partial lists [Q][tail ranges][k] and their counts behind the base's.
static bm_range_call bm_segment_call(const bm_range_call& call, const rag_bm25_index* sg, int Q, const bm25_topk_ws& w) {
    const size_t before = sg != call.seg ? (size_t)Q : 0, cnt = before * call.seg->n_ranges;      // (0: the base)
    bm_range_call c = call;
    c.seg = sg;
    c.out_ld = bm_total_docs(call.seg);
    c.plan = {w.plan.off + before * call.plan_t * (call.seg->n_ranges + 1), w.plan.meta + before * BM_PLAN_T};
    if (call.mode == 0) {
        c.part_key = w.part_key + cnt * call.k;
        c.part_row = w.part_row + cnt * call.k;
        c.part_cnt = w.part_cnt + cnt;
    }
    return c;
}
static void bm25_launch_plan(const bm_range_call& c, int Q, hipStream_t st) {
    const rag_bm25_index* s = c.seg;
    launch(s->wf != nullptr ? bm25_plan_kernel<true> : bm25_plan_kernel<false>, dim3((s->n_ranges + 1 + 255) / 256, Q), dim3(256), 0, st, s->meta,
           s->doc, s->range_tab, s->n_ranges, s->n_terms, c.term_ptr, c.terms, c.plan.off, c.plan.meta, c.plan_t, s->wf != nullptr ? c.qweights : nullptr);
}

// mode 1 over every segment: call.dense_out[Q][documents of the index] (+ the linear fusion's extras); each segment writes its own columns
static void bm25_launch_scores(const rag_ctx* h, const bm_range_call& call, int Q, const bm25_topk_ws& w, hipStream_t st) {
    for (const rag_bm25_index* sg : {call.seg, (const rag_bm25_index*)call.seg->tail.get()}) {
        if (sg == nullptr) continue;
        const bm_range_call c = bm_segment_call(call, sg, Q, w);
        bm25_launch_plan(c, Q, st);
        bm_launch_range(h, c, sg->n_ranges, Q, st);
    }
}

// folds the partial lists of the ranges [begin, end) of one segment into the running top-k (selection, or the bitonic sort)
static void bm25_launch_merge(const rag_ctx* h, const bm25_topk_ws& w, const uint64_t* part_key, const uint32_t* part_row, const int* part_cnt,
                              int nr, int begin, int end, int Q, int k, int first, int last, const bm25_topk_out& o, hipStream_t st) {
    if (k <= BMS_KMAX && !h->opt.bm25_sort_merge)
        hipLaunchKernelGGL(bm25_merge_select_kernel, dim3((Q + BMS_WAVES - 1) / BMS_WAVES), dim3(64 * BMS_WAVES), BMS_LDS_BYTES, st,
                           part_key, part_row, part_cnt, nr, begin, end, k, w.run_key, w.run_row, first, w.tau, last,
                           o.idmap, o.id_base, o.ids, o.rows, o.scores, o.raw_max, o.normalize, Q);
    else
        hipLaunchKernelGGL(bm25_merge_stage_kernel, dim3(Q), dim3(256), 0, st, part_key, part_row, part_cnt, nr, begin, end, k,
                           w.run_key, w.run_row, first, w.tau, last, o.idmap, o.id_base, o.ids, o.rows, o.scores,
                           o.raw_max, o.normalize);
}

// mode 0 over every segment, STAGED: ranges [0, first) get the exact per-range top-k; after every stage the running top-k
// of the query gives tau (k-th best so far), and the next stage - up to BM_STAGE_GROWTH x the ranges seen so far - only
// compacts keys >= tau. Expected survivors per stage ~ k * growth per query however large the shard is (a single
// threshold from 32768 docs left ~k/2 per range: 38 k entries per query to merge on a 12.5M-doc shard).
// The base runs these stages. The tail is ONE more thresholded stage: its rows come after every base row,
// so the running list's k-th key is the same lower bound for it as for a later base range (0 - everything passes - while the base
// held fewer than k documents), and its partial lists fold into the same running list. The last fold of the last segment finishes.
static void bm25_launch_topk(const rag_ctx* h, const bm_range_call& call, int Q, const bm25_topk_ws& w, const bm25_topk_out& o,
                             hipStream_t st) {
    const rag_bm25_index* ix = call.seg;
    const rag_bm25_index* tl = ix->tail.get();
    const int first_cfg = h->opt.bm25_first_ranges >= 1 && h->opt.bm25_first_ranges <= 16 ? h->opt.bm25_first_ranges : BM_FIRST_RANGES;
    int stage = 0;                                                    // stages run so far, over all segments
    for (const rag_bm25_index* sg : {ix, tl}) {
        if (sg == nullptr) continue;
        bm_range_call c = bm_segment_call(call, sg, Q, w);
        bm25_launch_plan(c, Q, st);
        const int nr = sg->n_ranges;
        const bool staged = sg == ix && nr > 2 * first_cfg && !h->opt.bm25_no_staging;
        for (int begin = 0; begin < nr; ++stage) {
            int end = !staged ? nr : (stage == 0 ? first_cfg : (int)std::min<int64_t>(nr, (int64_t)begin * BM_STAGE_GROWTH));
            if (staged && nr - end < end / 4) end = nr;                   // no tiny trailing stage
            c.range_begin = begin;
            c.tau_key = stage == 0 ? nullptr : w.tau;
            bm_launch_range(h, c, end - begin, Q, st);
            const int last = end == nr && (sg == tl || tl == nullptr);
            bm25_launch_merge(h, w, c.part_key, c.part_row, c.part_cnt, nr, begin, end, Q, call.k, stage == 0 ? 1 : 0, last, o, st);
            begin = end;
        }
    }
}

// the kept term-frequency plane (option bm25_keep_tf): the int32 frequencies of a load / an appended block as uint16
__global__ void bm25_tf16_kernel(const int32_t* __restrict__ tf, int64_t nnz, uint16_t* __restrict__ tf16) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < nnz) tf16[p] = (uint16_t)tf[p];
}
// a term frequency the uint16 plane cannot hold: RAG_ERR_ARG before anything is built
static int bm_check_tf16(rag_ctx* h, const int32_t* tf, int64_t nnz, const char* what) {
    for (int64_t p = 0; p < nnz; ++p)
        if (tf[p] < 0 || tf[p] > 65535) {
            h->err = std::string("bad argument: ") + what + ": a term frequency above 65535 does not fit the kept tf plane (option bm25_keep_tf)";
            return RAG_ERR_ARG;
        }
    return RAG_OK;
}

// ------------------------------------------------------------------------------------------------
void bm25_free(rag_ctx* h) {
    delete h->bm25;
    h->bm25 = nullptr;
}

// ---- the segment builder --------------------------------------------------------------------------------------------------
// Every way a segment comes to be - the load, an append (old tail ++ block), the fold (base ++ tail), a compaction's remap -
// runs the same steps and differs in step 6 alone:
//   1 bm_new_segment       a fresh rag_bm25_index: its place behind the documents before it, statistics and flags of its parent
//   2 bm_plan_terms        offsets -> term metadata + the plan of the bracket tables
//   3-5 bm_prepare_segment allocate, zero the padding, upload the metadata
//   6                      fill doc / w (or packed) / tf16 / dl: the caller's own kernels
//   7-8 bm_finish_segment  the bracket tables, the stream synchronise, the return code
// Everything new is built BESIDE the resident segments; the caller swaps it in once step 8 has succeeded, so a failure changes nothing.

// Who builds (the name in messages) and how a failed device allocation is reported: the load keeps dev_buf::alloc's RAG_ERR_HIP,
// the live operations (append, fold, compaction, refresh) report RAG_ERR_NOMEM. The two codes are part of the ABI: not unified.
template <class T>
static int bm_alloc(rag_ctx* h, dev_buf<T>& buf, size_t n, const char* what) {
    if (buf.alloc(h, std::max<size_t>(1, n)) == RAG_OK) return RAG_OK;
    (void)hipGetLastError();
    h->err = std::string(what) + ": out of device memory";
    return RAG_ERR_NOMEM;
}
struct bm_builder {
    rag_ctx* h;
    const char* what;
    bool nomem;
    template <class T>
    int alloc(dev_buf<T>& buf, size_t n) const { return nomem ? bm_alloc(h, buf, n, what) : buf.alloc(h, std::max<size_t>(1, n)); }
};

// Step 1. A segment of `docs` documents behind `prev_docs` documents of the index (0: a base). A tail numbers its documents from
// the start of the range the base ends in (see rag_bm25_index). Statistics, flags and counters come from `parent`, the base of
// the index it will belong to (null: the load sets its own) - the ONE place they are inherited.
static std::unique_ptr<rag_bm25_index> bm_new_segment(const rag_bm25_index* parent, int64_t prev_docs, int64_t docs, int64_t n_terms) {
    std::unique_ptr<rag_bm25_index> s(new rag_bm25_index());
    s->first = (int)(prev_docs % BM_RANGE);
    s->row0 = prev_docs - s->first;
    s->n_docs = s->first + docs;
    s->n_ranges = (int)((s->n_docs + BM_RANGE - 1) / BM_RANGE);
    s->n_terms = n_terms;
    if (parent != nullptr) {
        s->avgdl = parent->avgdl; s->k1 = parent->k1; s->b = parent->b;
        s->keep_tf = parent->keep_tf;
        s->normalize = parent->normalize;
        s->neg_idf_absmax = parent->neg_idf_absmax;
        s->appends = parent->appends; s->folds = parent->folds;
    }
    return s;
}

// offsets of the per-term concatenation A ++ B over V terms (A knows Va of them, B knows Vb)
static std::vector<int64_t> bm_merged_offsets(const int64_t* a, int64_t Va, const int64_t* b, int64_t Vb, int64_t V) {
    std::vector<int64_t> out((size_t)V + 1, 0);
    for (int64_t t = 0; t < V; ++t) out[(size_t)t + 1] = out[(size_t)t] + (t < Va ? a[t + 1] - a[t] : 0) + (t < Vb ? b[t + 1] - b[t] : 0);
    return out;
}

// Step 2. Offsets -> per-term metadata (null: only counted; idf may then be null too) and the number of bracket-table entries;
// -1 when a document frequency is negative or above max_df.
static int64_t bm_plan_terms(const int64_t* indptr, int64_t n_terms, int64_t n_docs, const double* idf, int64_t max_df,
                             std::vector<bm_term_meta>* meta_h) {
    const int64_t n_pad = (n_docs + BM_RANGE - 1) / BM_RANGE * BM_RANGE;
    if (meta_h) meta_h->resize((size_t)std::max<int64_t>(1, n_terms));
    int64_t n_tab = 0;
    for (int64_t t = 0; t < n_terms; ++t) {
        const int64_t df = indptr[t + 1] - indptr[t];
        if (df < 0 || df > max_df) return -1;
        int64_t e_t = 0;
        const int g = bm_plan_term(df, n_pad, &e_t);
        if (meta_h) (*meta_h)[(size_t)t] = {indptr[t], n_tab, idf ? idf[t] : 1.0, (int32_t)df, g};      // (no idf: the learned-sparse index)
        n_tab += e_t;
    }
    return n_tab;
}
// ... of a segment whose offsets are s->indptr_h (made here: cannot fail)
static void bm_plan_segment(rag_bm25_index* s, const double* idf, std::vector<bm_term_meta>& meta_h) {
    s->nnz = s->indptr_h[(size_t)s->n_terms];
    s->tab_entries = bm_plan_terms(s->indptr_h.data(), s->n_terms, s->n_docs, idf, s->n_docs, &meta_h);
}

// Steps 3-5. Allocates meta, range_tab, doc and the planes this segment carries (bm_planes), zeroes what the fill does not write,
// uploads the metadata (meta_h must stay alive until bm_finish_segment returns) and, for indptr_d, the offsets.
// THE PADDING: doc / w / packed / wf carry 8 zeroed postings past nnz - the scoring kernel reads 4 consecutive postings per thread,
// the bracket search 8 doc ids, without a bounds branch. dl starts zeroed: a tail's entries below `first` are never written.
struct bm_planes { bool w, packed, tf16, dl, indptr_d, wf; };
static int bm_prepare_segment(const bm_builder& B, rag_bm25_index* s, const std::vector<bm_term_meta>& meta_h, const bm_planes& pl) {
    rag_ctx* h = B.h;
    hipStream_t st = h->stream;
    const size_t nnz = (size_t)s->nnz, V = (size_t)s->n_terms;
    int rc;
    if ((rc = B.alloc(s->meta, meta_h.size()))) return rc;
    if ((rc = B.alloc(s->range_tab, (size_t)s->tab_entries))) return rc;
    if ((rc = B.alloc(s->doc, nnz + 8))) return rc;
    if (pl.w && (rc = B.alloc(s->w, nnz + 8))) return rc;
    if (pl.packed && (rc = B.alloc(s->packed, nnz + 8))) return rc;
    if (pl.wf && (rc = B.alloc(s->wf, nnz + 8))) return rc;
    if (pl.tf16 && (rc = B.alloc(s->tf16, nnz))) return rc;
    if (pl.dl && (rc = B.alloc(s->dl, (size_t)s->n_docs))) return rc;
    if (pl.indptr_d && (rc = B.alloc(s->indptr_d, V + 1))) return rc;
    HIP_TRY(h, hipMemsetAsync(s->doc + nnz, 0, 8 * sizeof(int32_t), st));
    if (pl.w) HIP_TRY(h, hipMemsetAsync(s->w + nnz, 0, 8 * sizeof(double), st));
    if (pl.packed) HIP_TRY(h, hipMemsetAsync(s->packed + nnz, 0, 8 * sizeof(uint32_t), st));
    if (pl.wf) HIP_TRY(h, hipMemsetAsync(s->wf + nnz, 0, 8 * sizeof(float), st));
    if (pl.dl) HIP_TRY(h, hipMemsetAsync(s->dl, 0, (size_t)s->n_docs * sizeof(int32_t), st));
    if (V) HIP_TRY(h, hipMemcpyAsync(s->meta, meta_h.data(), V * sizeof(bm_term_meta), hipMemcpyHostToDevice, st));
    if (pl.indptr_d) HIP_TRY(h, hipMemcpyAsync(s->indptr_d, s->indptr_h.data(), (V + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    return RAG_OK;
}

// Steps 7-8, given the result of everything enqueued so far: the bracket tables (s->doc is filled by now), then THE SYNCHRONISE,
// which runs after a failed enqueue too - the host arrays that queued copies read from stay alive until it returns.
static int bm_finish_segment(const bm_builder& B, rag_bm25_index* s, int rc) {
    rag_ctx* h = B.h;
    auto tables = [&]() -> int {
        bm_launch_1d(bm25_range_table_kernel, s->tab_entries, h->stream, s->meta, s->doc, s->n_terms, s->tab_entries, s->range_tab);
        HIP_TRY(h, hipGetLastError());
        return RAG_OK;
    };
    if (rc == RAG_OK && s->tab_entries) rc = tables();
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    if (rc) return rc;
    if (e2 != hipSuccess) {
        h->err = std::string(B.what) + ": " + hipGetErrorString(e2);
        return RAG_ERR_HIP;
    }
    return RAG_OK;
}

// host CSR -> device index (impacts + range table). Synchronous. *out receives the index on success only.
static int bm25_build(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len,
                      const double* idf, int64_t n_docs, int64_t n_terms, double avgdl, double k1, double b,
                      std::unique_ptr<rag_bm25_index>* out, bool keep_tf = false) {
    ARG_CHECK(h, n_docs > 0 && n_terms >= 0 && n_docs < 0x7fffffff, "bm25_load: bad sizes");
    ARG_CHECK(h, indptr && doc_len && (n_terms == 0 || idf), "bm25_load: null pointer");
    const int64_t nnz = n_terms ? indptr[n_terms] : 0;
    ARG_CHECK(h, nnz == 0 || (doc && tf), "bm25_load: null postings");
    if (keep_tf)
        if (int rc = bm_check_tf16(h, tf, nnz, "bm25_load")) return rc;
    const bm_builder B = {h, "bm25_load", false};
    std::unique_ptr<rag_bm25_index> ix = bm_new_segment(nullptr, 0, n_docs, n_terms);
    ix->keep_tf = keep_tf;
    ix->nnz = nnz; ix->avgdl = avgdl; ix->k1 = k1; ix->b = b;
    std::vector<bm_term_meta> meta_h;
    ix->tab_entries = bm_plan_terms(indptr, n_terms, n_docs, idf, n_docs, &meta_h);
    ARG_CHECK(h, ix->tab_entries >= 0, "bm25_load: indptr must be non-decreasing with at most n_docs postings per term");
    for (int64_t t = 0; t < n_terms; ++t)
        if (idf[t] < 0.0) ix->neg_idf_absmax = std::max(ix->neg_idf_absmax, -idf[t]);
    ix->indptr_h.assign(indptr, indptr + n_terms + 1);
    if (n_terms) ix->idf_h.assign(idf, idf + n_terms);
    hipStream_t st = h->stream;
    // code space of the packed postings: distinct term frequencies x distinct document lengths (host scans of tf[] and doc_len[])
    const int64_t code_cap = (int64_t)1 << (32 - BM_RANGE_LOG2);
    std::vector<uint32_t> tf_rank_h, dl_rank_of_doc_h;
    std::vector<double> tf_values_h, dl_values_h;
    bool packed_ok = nnz > 0 && h->opt.bm25_packed;      // opt-in: a third less HBM for the postings, a slower scoring loop
    if (packed_ok) {
        int32_t tf_max = 0, dl_max = 0;
        bool bad = false;
        for (int64_t p = 0; p < nnz; ++p) { const int32_t v = tf[p]; bad |= v <= 0; tf_max = v > tf_max ? v : tf_max; }
        for (int64_t d = 0; d < n_docs; ++d) { const int32_t v = doc_len[d]; bad |= v < 0; dl_max = v > dl_max ? v : dl_max; }
        packed_ok = !bad && tf_max < (1 << 24) && dl_max < (1 << 26);
        if (packed_ok) {
            std::vector<char> seen_tf((size_t)tf_max + 1, 0), seen_dl((size_t)dl_max + 1, 0);
            for (int64_t p = 0; p < nnz; ++p) seen_tf[(size_t)tf[p]] = 1;
            for (int64_t d = 0; d < n_docs; ++d) seen_dl[(size_t)doc_len[d]] = 1;
            tf_rank_h.assign((size_t)tf_max + 1, 0);
            std::vector<uint32_t> dl_rank((size_t)dl_max + 1, 0);
            for (int32_t v = 0; v <= tf_max; ++v) if (seen_tf[(size_t)v]) { tf_rank_h[(size_t)v] = (uint32_t)tf_values_h.size(); tf_values_h.push_back((double)v); }
            for (int32_t v = 0; v <= dl_max; ++v) if (seen_dl[(size_t)v]) { dl_rank[(size_t)v] = (uint32_t)dl_values_h.size(); dl_values_h.push_back((double)v); }
            ix->n_codes = (int64_t)tf_values_h.size() * (int64_t)dl_values_h.size();
            packed_ok = ix->n_codes <= code_cap;
            if (packed_ok) {
                dl_rank_of_doc_h.resize((size_t)n_docs);
                for (int64_t d = 0; d < n_docs; ++d) dl_rank_of_doc_h[(size_t)d] = dl_rank[(size_t)doc_len[d]];
            }
        }
    }
    if (!packed_ok) ix->n_codes = 0;
    // the fill's inputs: the index keeps none of them but what a refresh needs (its metadata carries the offsets and the idf)
    dev_buf<double> idf_d, tfv_d, dlv_d;
    dev_buf<int32_t> tfd;
    dev_buf<uint32_t> tfr_d, dlr_d;
    auto enqueue = [&]() -> int {
        int rc;
        // dl: the lengths the impacts are computed from; dropped again below unless a refresh will need them
        if ((rc = bm_prepare_segment(B, ix.get(), meta_h, {!packed_ok, packed_ok, keep_tf && !packed_ok, true, false}))) return rc;
        if ((rc = tfd.alloc(h, std::max<size_t>(1, nnz)))) return rc;
        if ((rc = idf_d.alloc(h, std::max<size_t>(1, n_terms)))) return rc;
        if (nnz) HIP_TRY(h, hipMemcpyAsync(ix->doc, doc, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (nnz) HIP_TRY(h, hipMemcpyAsync(tfd, tf, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (n_terms) HIP_TRY(h, hipMemcpyAsync(idf_d, idf, (size_t)n_terms * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(ix->dl, doc_len, (size_t)n_docs * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (packed_ok) {
            const uint32_t n_dl = (uint32_t)dl_values_h.size();
            if ((rc = ix->gtab.alloc(h, (size_t)ix->n_codes))) return rc;
            if ((rc = tfr_d.alloc(h, tf_rank_h.size()))) return rc;
            if ((rc = dlr_d.alloc(h, dl_rank_of_doc_h.size()))) return rc;
            if ((rc = tfv_d.alloc(h, tf_values_h.size()))) return rc;
            if ((rc = dlv_d.alloc(h, dl_values_h.size()))) return rc;
            HIP_TRY(h, hipMemcpyAsync(tfr_d, tf_rank_h.data(), tf_rank_h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(dlr_d, dl_rank_of_doc_h.data(), dl_rank_of_doc_h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(tfv_d, tf_values_h.data(), tf_values_h.size() * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(dlv_d, dl_values_h.data(), dl_values_h.size() * sizeof(double), hipMemcpyHostToDevice, st));
            bm_launch_1d(bm25_pack_kernel, nnz, st, ix->doc, tfd, tfr_d, dlr_d, nnz, n_dl, ix->packed);
            bm_launch_1d(bm25_gtab_kernel, ix->n_codes, st, tfv_d, dlv_d, ix->n_codes, n_dl, avgdl, k1, b, ix->gtab);
        } else if (nnz) {
            bm_launch_1d(bm25_impact_kernel<int32_t, bm_term_by_meta>, nnz, st, bm_term_by_meta{ix->meta, n_terms}, ix->doc, tfd, ix->dl, nnz,
                         avgdl, k1, b, idf_d, ix->w);
            if (keep_tf) bm_launch_1d(bm25_tf16_kernel, nnz, st, tfd, nnz, ix->tf16);
        }
        HIP_TRY(h, hipGetLastError());
        return RAG_OK;
    };
    if (int rc = bm_finish_segment(B, ix.get(), enqueue())) return rc;
    if (!keep_tf) ix->dl.reset();
    else if (packed_ok) {                    // a packed base is refreshed from the two value tables of its impact table
        ix->tfv = std::move(tfv_d);
        ix->dlv = std::move(dlv_d);
        ix->n_dl = (uint32_t)dl_values_h.size();
    }
    *out = std::move(ix);
    return RAG_OK;
}

int bm25_load_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len,
                   const double* idf, int64_t n_docs, int64_t n_terms, double avgdl, double k1, double b) {
    std::unique_ptr<rag_bm25_index> ix;
    const int rc = bm25_build(h, indptr, doc, tf, doc_len, idf, n_docs, n_terms, avgdl, k1, b, &ix, h->opt.bm25_keep_tf != 0);
    if (rc) return rc;
    bm25_free(h);
    h->bm25 = ix.release();
    h->bm25_stale = false;
    h->bm25_compacted = false;
    return RAG_OK;
}

// ---- appendable postings --------------------------------------------------------------------------------------------------
// Per-term concatenation A ++ B into a new posting array, one thread per DESTINATION posting: its term comes from the
// destination's offsets (bm_term_by_offsets), its place j inside the term's list picks the source - the first
// a_df postings come from A (an index: per-term metadata), the rest from B (a CSR: offsets). Document numbers are shifted
// into the destination's numbering. The append runs it as old tail ++ block, the fold as base ++ tail. W: the posting's weight
// plane - float64 impacts (BM25) or the float32 weights of the learned-sparse index - copied as stored bits.
template <class W>
__global__ void bm25_concat_kernel(const int64_t* __restrict__ out_indptr, int64_t n_terms, int64_t nnz,
                                   const bm_term_meta* __restrict__ a_meta, int64_t a_terms, const int32_t* __restrict__ a_doc,
                                   const W* __restrict__ a_w, const int64_t* __restrict__ b_indptr,
                                   const int32_t* __restrict__ b_doc, const W* __restrict__ b_w, int32_t b_shift,
                                   int32_t* __restrict__ doc_out, W* __restrict__ w_out,
                                   const uint16_t* __restrict__ a_tf, const uint16_t* __restrict__ b_tf, uint16_t* __restrict__ tf_out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const int64_t lo = bm_term_by_offsets{out_indptr, n_terms}(p);
    const int64_t j = p - out_indptr[lo];
    int64_t a_df = 0, a_post = 0;
    if (lo < a_terms) {
        a_df = a_meta[lo].df;
        a_post = a_meta[lo].post;
    }
    if (j < a_df) {
        doc_out[p] = a_doc[a_post + j];
        w_out[p] = a_w[a_post + j];
        if (tf_out != nullptr) tf_out[p] = a_tf[a_post + j];       // (uniform) the kept term frequencies travel with the impacts
    } else {
        const int64_t s = b_indptr[lo] + (j - a_df);
        doc_out[p] = b_doc[s] + b_shift;
        w_out[p] = b_w[s];
        if (tf_out != nullptr) tf_out[p] = b_tf[s];
    }
}

// Default of option bm25_tail_fold (0): the tail size, in documents, past which an append folds by itself. The tail costs every
// search one more plan + scoring + fold launch and every append a rebuild of the whole tail, the fold one pass over all postings.
// Measured at 1M documents (profiles/live_bm25_1M.json): a 5 % tail adds 0.1 ms to a 0.94 ms Q = 256 search and 1 ms
// to an append, the fold takes 5 ms - all small, so the default stays where it was.
static int64_t bm_default_fold_docs(int64_t base_docs) { return std::max<int64_t>(32 * BM_RANGE, base_docs / 16); }

// The handle's two resident indexes - the BM25 postings and the learned-sparse postings - as ONE kind of slot: the index, its two
// staleness flags, its fold option and its names in messages. Append, fold, segment statistics and the compaction's remap are
// written once over a slot; what differs per slot is how an appended block's weight plane comes to be (impacts computed from
// term frequencies / float32 weights uploaded as they are) and the plane's type (bm_weights).
struct bm_slot {
    rag_bm25_index*& ix;
    bool& stale;                 // rows were inserted or compacted since the postings were aligned
    bool& compacted;             // ... and a plain compaction was among them: only a reload helps
    int fold_opt;                // option bm25_tail_fold / sparse_tail_fold
    const char* append_name;
    const char* fold_name;
    const char* stats_name;
};
static bm_slot bm_slot_bm25(rag_ctx* h) {
    return {h->bm25, h->bm25_stale, h->bm25_compacted, h->opt.bm25_tail_fold, "bm25_append", "bm25_fold", "bm25_segment_stats"};
}
static bm_slot bm_slot_sparse(rag_ctx* h) {
    return {h->sparse, h->sparse_stale, h->sparse_compacted, h->opt.sparse_tail_fold, "sparse_append", "sparse_fold", "sparse_segment_stats"};
}
template <class W> static dev_buf<W>& bm_weights(rag_bm25_index* s);
template <> dev_buf<double>& bm_weights<double>(rag_bm25_index* s) { return s->w; }
template <> dev_buf<float>& bm_weights<float>(rag_bm25_index* s) { return s->wf; }
// terms the index knows, loaded and appended (the BM25 postings keep an idf for each)
static int64_t bm_known_terms(const rag_bm25_index* ix) {
    return ix->wf != nullptr ? std::max(ix->n_terms, ix->tail ? ix->tail->n_terms : (int64_t)0) : (int64_t)ix->idf_h.size();
}

static int bm_fold(rag_ctx* h, const bm_slot& S);

// Host checks of an appended block, before anything is built: the next n_new rows behind the covered ones, a term-major CSR over
// V >= the known terms, documents ascending inside a term and relative to the block. ptrs_ok / planes_ok: the caller's further
// arrays (document lengths, new idf values / the postings' value plane) are present.
static int bm_check_block(rag_ctx* h, const char* who, const rag_bm25_index* ix, const int64_t* indptr, const int32_t* doc, int64_t n_new,
                          int64_t V, bool ptrs_ok, bool planes_ok) {
    const std::string w = std::string(who) + ": ";
    const int64_t known = bm_known_terms(ix), covered = bm_total_docs(ix);
    ARG_CHECK(h, n_new >= 1 && covered + n_new < 0x7fffffff, w + "n_docs_new must be >= 1 (and the index stay under 2^31 documents)");
    ARG_CHECK(h, V >= known && V < 0x7fffffff, w + "n_terms_total may not shrink");
    ARG_CHECK(h, indptr && ptrs_ok, w + "null pointer");
    ARG_CHECK(h, !h->index_loaded || covered + n_new <= h->n_rows, w + "the block would cover more rows than the index has");
    ARG_CHECK(h, indptr[0] == 0, w + "indptr must start at 0");
    for (int64_t t = 0; t < V; ++t) {
        const int64_t df = indptr[t + 1] - indptr[t];
        ARG_CHECK(h, df >= 0 && df <= n_new, w + "indptr must be non-decreasing with at most n_docs_new postings per term");
    }
    ARG_CHECK(h, indptr[V] == 0 || (doc && planes_ok), w + "null postings");
    for (int64_t t = 0; t < V; ++t)            // the block's documents become device addresses: in range, ascending inside a term
        for (int64_t p = indptr[t]; p < indptr[t + 1]; ++p)
            ARG_CHECK(h, doc[p] >= 0 && doc[p] < n_new && (p == indptr[t] || doc[p] > doc[p - 1]),
                      w + "doc must be ascending inside a term and below n_docs_new");
    return RAG_OK;
}

// The new tail = old tail ++ block, built beside the old one: *out receives it on success only. `fill(b_indptr, b_doc, &b_w,
// &b_tf16)` enqueues the block's weight plane (and, under keep_tf, its uint16 term frequencies) on the device; the buffers it
// allocates belong to the caller and outlive this call's synchronise. idf: one value per term of V, or null (every idf 1).
// The block's offsets and document plane are uploaded from `indptr` / `doc`, unless the caller has them on the device already
// (indptr_dev / doc_dev, rag_sparse_append_dev): then `doc` is not read and `indptr` is the host copy the plan is made from.
template <class W, class Fill>
static int bm_build_tail(rag_ctx* h, const bm_builder& B, const rag_bm25_index* ix, const int64_t* indptr, const int32_t* doc,
                         const int32_t* doc_len, int64_t n_new, int64_t V, const double* idf, Fill&& fill,
                         std::unique_ptr<rag_bm25_index>* out, const int64_t* indptr_dev = nullptr, const int32_t* doc_dev = nullptr) {
    constexpr bool F32 = std::is_same<W, float>::value;
    rag_bm25_index* ot = ix->tail.get();
    const bool keep = ix->keep_tf;
    const int64_t nnz_b = indptr[V], Vo = ot ? ot->n_terms : 0;
    std::unique_ptr<rag_bm25_index> nt = bm_new_segment(ix, ix->n_docs, ix->tail_docs + n_new, V);
    nt->indptr_h = bm_merged_offsets(ot ? ot->indptr_h.data() : nullptr, Vo, indptr, V, V);
    std::vector<bm_term_meta> meta_h;
    bm_plan_segment(nt.get(), idf, meta_h);
    hipStream_t st = h->stream;
    dev_buf<int64_t> b_indptr;
    dev_buf<int32_t> b_doc;
    auto enqueue = [&]() -> int {
        int rc;
        if ((rc = bm_prepare_segment(B, nt.get(), meta_h, {!F32, false, keep, keep, true, F32}))) return rc;
        if (keep) {                          // the tail's document lengths: the old tail's, then the block's (its tf plane: concatenated below)
            if (ot && ix->tail_docs)
                HIP_TRY(h, hipMemcpyAsync(nt->dl + nt->first, ot->dl + ot->first, (size_t)ix->tail_docs * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(nt->dl + nt->first + ix->tail_docs, doc_len, (size_t)n_new * 4, hipMemcpyHostToDevice, st));
        }
        const int64_t* bi = indptr_dev;
        const int32_t* bd = doc_dev;
        if (bi == nullptr) {                 // a host block: its two planes go up here
            if ((rc = bm_alloc(h, b_indptr, (size_t)V + 1, B.what))) return rc;
            if ((rc = bm_alloc(h, b_doc, (size_t)nnz_b, B.what))) return rc;
            HIP_TRY(h, hipMemcpyAsync(b_indptr, indptr, (size_t)(V + 1) * 8, hipMemcpyHostToDevice, st));
            if (nnz_b) HIP_TRY(h, hipMemcpyAsync(b_doc, doc, (size_t)nnz_b * 4, hipMemcpyHostToDevice, st));
            bi = b_indptr.get();
            bd = b_doc.get();
        }
        const W* b_w = nullptr;
        const uint16_t* b_tf16 = nullptr;
        if ((rc = fill(bi, bd, &b_w, &b_tf16))) return rc;
        if (nt->nnz)
            bm_launch_1d(bm25_concat_kernel<W>, nt->nnz, st, nt->indptr_d, V, nt->nnz, ot ? ot->meta.get() : nullptr, Vo,
                         ot ? ot->doc.get() : nullptr, ot ? bm_weights<W>(ot).get() : nullptr, bi, bd, b_w,
                         (int32_t)(nt->first + ix->tail_docs), nt->doc, bm_weights<W>(nt.get()), ot ? ot->tf16.get() : nullptr, b_tf16,
                         nt->tf16);
        HIP_TRY(h, hipGetLastError());
        return RAG_OK;
    };
    if (int rc = bm_finish_segment(B, nt.get(), enqueue())) return rc;
    *out = std::move(nt);
    return RAG_OK;
}

// The commit of an append: the new tail replaces the old one; the postings are aligned again when every row is covered and only
// inserts came between (a plain compaction renumbers rows: reload); then the automatic fold of the slot's option.
static void bm_append_commit(rag_ctx* h, const bm_slot& S, std::unique_ptr<rag_bm25_index> nt, int64_t n_new) {
    rag_bm25_index* ix = S.ix;
    ix->tail = std::move(nt);
    ix->tail_docs += n_new;
    ix->appends++;
    if (S.stale && !S.compacted && h->index_loaded && bm_total_docs(ix) == h->n_rows) S.stale = false;
    const int64_t fold_at = S.fold_opt > 0 ? S.fold_opt : (S.fold_opt == 0 ? bm_default_fold_docs(ix->n_docs) : -1);
    if (fold_at > 0 && ix->tail_docs > fold_at && ix->packed == nullptr) {
        if (bm_fold(h, S) != RAG_OK) h->err.clear();         // the append itself is done; the tail simply stays (e.g. no memory for the merged arrays)
    }
}

int bm25_append_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len,
                     const double* idf_new, int64_t n_new, int64_t n_terms_total) {
    if (!h->bm25) {
        h->err = "bm25_append: no postings loaded (rag_bm25_load_host first)";
        return RAG_ERR_STATE;
    }
    const bm_slot S = bm_slot_bm25(h);
    rag_bm25_index* ix = h->bm25;
    const int64_t known = (int64_t)ix->idf_h.size(), V = n_terms_total;
    if (int rc = bm_check_block(h, S.append_name, ix, indptr, doc, n_new, V, doc_len && (V <= known || idf_new), tf != nullptr)) return rc;
    const int64_t nnz_b = indptr[V];
    const bool keep = ix->keep_tf;
    if (keep)
        if (int rc = bm_check_tf16(h, tf, nnz_b, "bm25_append")) return rc;
    std::vector<double> idf_all(ix->idf_h);
    idf_all.insert(idf_all.end(), idf_new, idf_new + (V - known));
    double neg = ix->neg_idf_absmax;
    for (int64_t t = known; t < V; ++t) if (idf_all[(size_t)t] < 0.0) neg = std::max(neg, -idf_all[(size_t)t]);
    const bm_builder B = {h, S.append_name, true};
    const char* what = B.what;
    hipStream_t st = h->stream;
    dev_buf<int32_t> b_tf, b_dl;
    dev_buf<double> b_w, idf_d;
    dev_buf<uint16_t> b_tf16;
    // the block's impacts: the arithmetic of the load, with the FROZEN avgdl and the concatenated idf table
    auto fill = [&](const int64_t* b_indptr, const int32_t* b_doc, const double** w_out, const uint16_t** tf16_out) -> int {
        int rc;
        if (keep && (rc = bm_alloc(h, b_tf16, (size_t)nnz_b, what))) return rc;
        if ((rc = bm_alloc(h, b_tf, (size_t)nnz_b, what))) return rc;
        if ((rc = bm_alloc(h, b_w, (size_t)nnz_b, what))) return rc;
        if ((rc = bm_alloc(h, b_dl, (size_t)n_new, what))) return rc;
        if ((rc = bm_alloc(h, idf_d, (size_t)V, what))) return rc;
        if (V) HIP_TRY(h, hipMemcpyAsync(idf_d, idf_all.data(), (size_t)V * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipMemcpyAsync(b_dl, doc_len, (size_t)n_new * 4, hipMemcpyHostToDevice, st));
        if (nnz_b) {
            HIP_TRY(h, hipMemcpyAsync(b_tf, tf, (size_t)nnz_b * 4, hipMemcpyHostToDevice, st));
            bm_launch_1d(bm25_impact_kernel<int32_t, bm_term_by_offsets>, nnz_b, st, bm_term_by_offsets{b_indptr, V}, b_doc, b_tf, b_dl, nnz_b,
                         ix->avgdl, ix->k1, ix->b, idf_d, b_w);
            if (keep) bm_launch_1d(bm25_tf16_kernel, nnz_b, st, b_tf, nnz_b, b_tf16);
        }
        *w_out = b_w;
        *tf16_out = b_tf16;
        return RAG_OK;
    };
    std::unique_ptr<rag_bm25_index> nt;
    if (int rc = bm_build_tail<double>(h, B, ix, indptr, doc, doc_len, n_new, V, idf_all.data(), fill, &nt)) return rc;
    ix->idf_h = std::move(idf_all);
    ix->neg_idf_absmax = neg;
    bm_append_commit(h, S, std::move(nt), n_new);
    return RAG_OK;
}

// base ++ tail -> one base, on the device; results are bit-identical before and after (the same impacts, per-term lists in the
// same order, tables from the same builders)
static int bm_fold(rag_ctx* h, const bm_slot& S) {
    if (!S.ix) {
        h->err = std::string(S.fold_name) + ": no postings loaded";
        return RAG_ERR_STATE;
    }
    rag_bm25_index* ix = S.ix;
    rag_bm25_index* tl = ix->tail.get();
    if (tl == nullptr) return RAG_OK;
    if (ix->packed != nullptr) {
        h->err = "bm25_fold: the base postings are packed (option bm25_packed): their code table cannot absorb new (tf, length) pairs; "
                 "reload to merge";
        return RAG_ERR_STATE;
    }
    const bm_builder B = {h, S.fold_name, true};
    const int64_t V = std::max(tl->n_terms, ix->n_terms), Vb = ix->n_terms, Vt = tl->n_terms;
    const bool keep = ix->keep_tf, f32 = ix->wf != nullptr;
    std::unique_ptr<rag_bm25_index> nb = bm_new_segment(ix, 0, bm_total_docs(ix), V);
    nb->indptr_h = bm_merged_offsets(ix->indptr_h.data(), Vb, tl->indptr_h.data(), Vt, V);
    std::vector<bm_term_meta> meta_h;
    bm_plan_segment(nb.get(), ix->idf_h.empty() ? nullptr : ix->idf_h.data(), meta_h);
    hipStream_t st = h->stream;
    auto enqueue = [&]() -> int {
        // (indptr_d: the concatenation's destination offsets; only a tail keeps them, see the commit)
        if (int rc = bm_prepare_segment(B, nb.get(), meta_h, {!f32, false, keep, keep, true, f32})) return rc;
        if (keep) {                          // the documents' lengths: the base's, then the tail's own
            HIP_TRY(h, hipMemcpyAsync(nb->dl, ix->dl, (size_t)ix->n_docs * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(nb->dl + ix->n_docs, tl->dl + tl->first, (size_t)ix->tail_docs * 4, hipMemcpyDeviceToDevice, st));
        }
        if (nb->nnz && f32)
            bm_launch_1d(bm25_concat_kernel<float>, nb->nnz, st, nb->indptr_d, V, nb->nnz, ix->meta, Vb, ix->doc, ix->wf, tl->indptr_d, tl->doc,
                         tl->wf, (int32_t)tl->row0, nb->doc, nb->wf, ix->tf16, tl->tf16, nb->tf16);
        else if (nb->nnz)
            bm_launch_1d(bm25_concat_kernel<double>, nb->nnz, st, nb->indptr_d, V, nb->nnz, ix->meta, Vb, ix->doc, ix->w, tl->indptr_d, tl->doc,
                         tl->w, (int32_t)tl->row0, nb->doc, nb->w, ix->tf16, tl->tf16, nb->tf16);
        HIP_TRY(h, hipGetLastError());
        return RAG_OK;
    };
    if (int rc = bm_finish_segment(B, nb.get(), enqueue())) return rc;
    // commit
    nb->indptr_d.reset();
    nb->idf_h = std::move(ix->idf_h);
    nb->folds = ix->folds + 1;
    delete ix;                               // the old base, its tail and their workspaces
    S.ix = nb.release();
    return RAG_OK;
}
int bm25_fold(rag_ctx* h) { return bm_fold(h, bm_slot_bm25(h)); }
int sparse_fold(rag_ctx* h) { return bm_fold(h, bm_slot_sparse(h)); }

// ---- postings through a compaction (rag_index_compact_bm25) ---------------------------------------------------------------
// The compaction's row map is monotone on the live rows, so a STABLE stream compaction of a segment's whole posting array keeps
// it term-major with ascending documents per term: postings of deleted rows drop out, the others get their new document number
// and keep their impact (or the code bits of a packed posting). Three kernels over tiles of BM_CP_TILE consecutive postings; the
// exclusive scan of the tile counts is a host round trip (4 B per 2048 postings), like the one of the rows' own tile counts.
#define BM_CP_TILE 2048
#define BM_CP_WORDS (BM_CP_TILE / 64)

// keep pass: bit p of `mask` = posting p survives (its row has a new number); tile_cnt[tile] = survivors of the tile. `mask`
// holds BM_CP_WORDS words for every tile, also the last, partial one.
__global__ __launch_bounds__(256) void bm25_compact_keep_kernel(const int32_t* __restrict__ doc, int64_t nnz, const int64_t* __restrict__ row_map,
                                                                 int64_t n_map, int64_t row0, unsigned long long* __restrict__ mask,
                                                                 int* __restrict__ tile_cnt) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * BM_CP_TILE;
    int c = 0;
#pragma unroll
    for (int j = 0; j < BM_CP_TILE / 256; ++j) {
        const int64_t p = p0 + j * 256 + tid;
        bool keep = false;
        if (p < nnz) {
            const int64_t r = row0 + doc[p];
            keep = (uint64_t)r < (uint64_t)n_map && row_map[r] >= 0;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) {
            mask[(p0 >> 6) + j * 4 + w] = m;
            c += __popcll(m);
        }
    }
    if (lane == 0) wsum[w] = c;
    __syncthreads();
    if (tid == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// new posting offsets, one thread per entry of indptr: survivors before posting indptr[t] = the tile's offset + the set bits of
// the tile's mask words before it (at most BM_CP_WORDS words, not a walk over postings)
__global__ void bm25_compact_indptr_kernel(const int64_t* __restrict__ indptr, int64_t n_entries, int64_t nnz, int64_t nnz_new,
                                           const unsigned long long* __restrict__ mask, const int64_t* __restrict__ tile_off,
                                           int64_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_entries) return;
    const int64_t p = indptr[t];
    if (p >= nnz) {
        out[t] = nnz_new;
        return;
    }
    const int64_t tile = p / BM_CP_TILE, word = p >> 6;
    int64_t c = tile_off[tile];
    for (int64_t i = tile * BM_CP_WORDS; i < word; ++i) c += __popcll(mask[i]);
    out[t] = c + __popcll(mask[word] & ((1ull << (p & 63)) - 1ull));
}

// scatter pass: survivor p goes to tile_off[tile] + its rank inside the tile (set bits of the mask before it), renumbered into
// the new segment (new local document = new row - new_row0). A tile's destinations are contiguous. PACKED: the 4-byte posting
// keeps its code bits and gets the low bits of the new document number (a base: new_row0 = 0). W: the weight plane of an unpacked
// segment, float64 impacts or the learned-sparse index's float32 weights, moved as stored bits.
template <bool PACKED, class W>
__global__ __launch_bounds__(256) void bm25_compact_scatter_kernel(const int32_t* __restrict__ doc, const W* __restrict__ w,
                                                                    const uint32_t* __restrict__ packed, const int64_t* __restrict__ row_map,
                                                                    int64_t row0, int64_t new_row0, const unsigned long long* __restrict__ mask,
                                                                    const int64_t* __restrict__ tile_off, int32_t* __restrict__ doc_out,
                                                                    W* __restrict__ w_out, uint32_t* __restrict__ packed_out,
                                                                    const uint16_t* __restrict__ tf, uint16_t* __restrict__ tf_out) {
    __shared__ int pre[BM_CP_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long* mw = mask + (int64_t)blockIdx.x * BM_CP_WORDS;
    if (wv == 0) {                           // exclusive prefix of the words' survivor counts (32 words: half a wave)
        const int c = lane < BM_CP_WORDS ? __popcll(mw[lane]) : 0;
        int s = c;
#pragma unroll
        for (int d = 1; d < BM_CP_WORDS; d <<= 1) {
            const int v = __shfl_up(s, d);
            if (lane >= d) s += v;
        }
        if (lane < BM_CP_WORDS) pre[lane] = s - c;
    }
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * BM_CP_TILE, base = tile_off[blockIdx.x];
#pragma unroll
    for (int j = 0; j < BM_CP_TILE / 256; ++j) {
        const int k = j * 4 + wv;
        const unsigned long long m = mw[k];
        if (!((m >> lane) & 1ull)) continue;
        const int64_t p = p0 + j * 256 + tid;
        const int64_t dst = base + pre[k] + __popcll(m & ((1ull << lane) - 1ull));
        const int32_t nd = (int32_t)(row_map[row0 + doc[p]] - new_row0);
        doc_out[dst] = nd;
        if (PACKED) packed_out[dst] = (packed[p] & ~(uint32_t)(BM_RANGE - 1)) | ((uint32_t)nd & (BM_RANGE - 1));
        else w_out[dst] = w[p];
        if (!PACKED && tf_out != nullptr) tf_out[dst] = tf[p];      // (uniform) the kept term frequency: same mask, same offset
    }
}

// the kept document lengths through the row map: old local document d of a segment -> its new local number, when it survives
__global__ void bm25_compact_dl_kernel(const int32_t* __restrict__ dl, int64_t first, int64_t n_docs, int64_t row0,
                                       const int64_t* __restrict__ row_map, int64_t n_map, int64_t new_row0, int64_t new_docs,
                                       int32_t* __restrict__ dl_out) {
    const int64_t d = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_docs || row0 + d >= n_map) return;
    const int64_t nd = row_map[row0 + d] - new_row0;
    if (nd >= 0 && nd < new_docs) dl_out[nd] = dl[d];             // (a deleted row maps to -1: nd < 0)
}

// One segment `os` -> `ns` (a bm_new_segment; the old one is not touched):
// row_map[os->row0 + local document] is the new row or -1, rows at or past n_map have no entry. Synchronous.
static int bm_remap_segment(rag_ctx* h, const rag_bm25_index* os, rag_bm25_index* ns, const std::vector<double>& idf,
                            const int64_t* row_map, int64_t n_map, bool keep_indptr_d) {
    const bool f32 = os->wf != nullptr;     // a learned-sparse segment (every idf 1: `idf` is empty)
    const bm_builder B = {h, f32 ? "compact_live (sparse postings)" : "compact_bm25", true};
    const char* what = B.what;
    const int64_t V = os->n_terms, nnz = os->nnz, tiles = (nnz + BM_CP_TILE - 1) / BM_CP_TILE;
    const bool packed = os->packed != nullptr, keep = os->keep_tf;
    hipStream_t st = h->stream;
    ns->indptr_h.assign((size_t)V + 1, 0);
    dev_buf<unsigned long long> mask;
    dev_buf<int> tile_cnt;
    dev_buf<int64_t> tile_off, indptr_old, indptr_new;
    std::vector<int> cnt((size_t)tiles);
    std::vector<int64_t> off((size_t)tiles);
    std::vector<bm_term_meta> meta_h;
    auto enqueue = [&]() -> int {
        int rc;
        if (nnz > 0) {                       // keep pass, then the new offsets (two host round trips)
            int64_t nnz_new = 0;
            if ((rc = bm_alloc(h, mask, (size_t)tiles * BM_CP_WORDS, what))) return rc;
            if ((rc = bm_alloc(h, tile_cnt, (size_t)tiles, what))) return rc;
            if ((rc = bm_alloc(h, tile_off, (size_t)tiles, what))) return rc;
            if ((rc = bm_alloc(h, indptr_old, (size_t)V + 1, what))) return rc;
            if ((rc = bm_alloc(h, indptr_new, (size_t)V + 1, what))) return rc;
            hipLaunchKernelGGL(bm25_compact_keep_kernel, dim3((unsigned)tiles), dim3(256), 0, st, os->doc.get(), nnz, row_map, n_map, os->row0,
                               mask.get(), tile_cnt.get());
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(cnt.data(), tile_cnt, (size_t)tiles * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
            for (int64_t t = 0; t < tiles; ++t) {
                off[(size_t)t] = nnz_new;
                nnz_new += cnt[(size_t)t];
            }
            HIP_TRY(h, hipMemcpyAsync(tile_off, off.data(), (size_t)tiles * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(indptr_old, os->indptr_h.data(), (size_t)(V + 1) * 8, hipMemcpyHostToDevice, st));
            bm_launch_1d(bm25_compact_indptr_kernel, V + 1, st, indptr_old, V + 1, nnz, nnz_new, mask, tile_off, indptr_new);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(ns->indptr_h.data(), indptr_new, (size_t)(V + 1) * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(h, hipStreamSynchronize(st));
        }
        bm_plan_segment(ns, idf.empty() ? nullptr : idf.data(), meta_h);
        if ((rc = bm_prepare_segment(B, ns, meta_h, {!packed && !f32, packed, keep && !packed, keep, keep_indptr_d, f32}))) return rc;
        if (packed) {                        // the code table is shared by every posting that survives: copied as it is
            if ((rc = bm_alloc(h, ns->gtab, os->gtab.size(), what))) return rc;
            ns->n_codes = os->n_codes;
            HIP_TRY(h, hipMemcpyAsync(ns->gtab, os->gtab, os->gtab.size() * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (keep) {                      // ... and so are the value tables it is rebuilt from
                if ((rc = bm_alloc(h, ns->tfv, os->tfv.size(), what))) return rc;
                if ((rc = bm_alloc(h, ns->dlv, os->dlv.size(), what))) return rc;
                ns->n_dl = os->n_dl;
                HIP_TRY(h, hipMemcpyAsync(ns->tfv, os->tfv, os->tfv.size() * sizeof(double), hipMemcpyDeviceToDevice, st));
                HIP_TRY(h, hipMemcpyAsync(ns->dlv, os->dlv, os->dlv.size() * sizeof(double), hipMemcpyDeviceToDevice, st));
            }
        }
        const int64_t own = os->n_docs - os->first;
        if (keep && own > 0)
            bm_launch_1d(bm25_compact_dl_kernel, own, st, os->dl, (int64_t)os->first, os->n_docs, os->row0, row_map, n_map, ns->row0,
                         ns->n_docs, ns->dl);
        if (nnz > 0 && f32)
            hipLaunchKernelGGL((bm25_compact_scatter_kernel<false, float>), dim3((unsigned)tiles), dim3(256), 0, st, os->doc.get(), os->wf.get(),
                               os->packed.get(), row_map, os->row0, ns->row0, mask.get(), tile_off.get(), ns->doc.get(), ns->wf.get(),
                               ns->packed.get(), os->tf16.get(), ns->tf16.get());
        else if (nnz > 0)
            hipLaunchKernelGGL((packed ? bm25_compact_scatter_kernel<true, double> : bm25_compact_scatter_kernel<false, double>),
                               dim3((unsigned)tiles), dim3(256), 0, st, os->doc.get(), os->w.get(), os->packed.get(), row_map, os->row0,
                               ns->row0, mask.get(), tile_off.get(), ns->doc.get(), ns->w.get(), ns->packed.get(), os->tf16.get(),
                               ns->tf16.get());
        HIP_TRY(h, hipGetLastError());
        return RAG_OK;
    };
    return bm_finish_segment(B, ns, enqueue());
}

int64_t bm25_base_docs(const rag_bm25_index* ix) { return ix ? ix->n_docs : 0; }
int64_t bm25_covered_docs(const rag_bm25_index* ix) { return ix ? bm_total_docs(ix) : 0; }

// The postings as they will be after the compaction whose device row map is `row_map` (entries for the covered rows), built
// BESIDE the resident ones: *out is handed to bm25_compact_commit once the rows have moved, or to bm25_compact_discard.
// base_live / covered_live = live rows among the base's rows / among all covered rows. Base and tail are remapped SEPARATELY (no
// fold: a packed base cannot absorb its tail, and one rule serves both forms); the new tail hangs behind the new base exactly
// as bm25_append_host would have put it (row0 = the base's last range, first = base documents in that range). A tail without
// survivors is dropped; a base without survivors is replaced by the remapped tail (always the (doc, impact) form). *out stays
// null when no covered row survives: there is nothing to keep, the caller falls back to the plain compaction. ix: the BM25
// postings (rag_index_compact_bm25, rag_index_compact_live) or the learned-sparse postings (rag_index_compact_live).
int bm25_compact_prepare(rag_ctx* h, const rag_bm25_index* ix, const int64_t* row_map, int64_t base_live, int64_t covered_live,
                         rag_bm25_index** out) {
    *out = nullptr;
    const rag_bm25_index* tl = ix->tail.get();
    const int64_t n_map = bm_total_docs(ix), tail_live = covered_live - base_live;
    if (covered_live <= 0) return RAG_OK;
    const int64_t V = ix->n_terms, Vt = tl ? tl->n_terms : 0;
    std::unique_ptr<rag_bm25_index> nb;
    int rc;
    if (base_live > 0) {
        nb = bm_new_segment(ix, 0, base_live, V);
        if ((rc = bm_remap_segment(h, ix, nb.get(), ix->idf_h, row_map, n_map, false))) return rc;
        if (tl != nullptr && tail_live > 0) {
            std::unique_ptr<rag_bm25_index> nt = bm_new_segment(ix, base_live, tail_live, Vt);
            if ((rc = bm_remap_segment(h, tl, nt.get(), ix->idf_h, row_map, n_map, true))) return rc;
            nb->tail = std::move(nt);
            nb->tail_docs = tail_live;
        }
    } else {
        nb = bm_new_segment(ix, 0, tail_live, Vt);
        if ((rc = bm_remap_segment(h, tl, nb.get(), ix->idf_h, row_map, n_map, false))) return rc;
    }
    nb->idf_h = ix->idf_h;
    *out = nb.release();
    return RAG_OK;
}

void bm25_compact_discard(rag_bm25_index* nb) { delete nb; }

void bm25_compact_commit(rag_bm25_index** slot, rag_bm25_index* nb) {
    delete *slot;                            // the old base, its tail and their workspaces
    *slot = nb;
}

// HBM bytes of one segment's arrays
static int64_t bm_segment_bytes(const rag_bm25_index* s) {
    return (int64_t)(s->doc.size() * 4 + s->w.size() * 8 + s->wf.size() * 4 + s->packed.size() * 4 + s->meta.size() * sizeof(bm_term_meta) +
                     s->range_tab.size() * 4 + s->indptr_d.size() * 8 + s->tf16.size() * 2 + s->dl.size() * 4);
}

static int bm_segment_stats(rag_ctx* h, const bm_slot& S, rag_bm25_segments* out) {
    ARG_CHECK(h, out != nullptr, std::string(S.stats_name) + ": null output");
    if (!S.ix) {
        h->err = std::string(S.stats_name) + ": no postings loaded";
        return RAG_ERR_STATE;
    }
    const rag_bm25_index* ix = S.ix;
    const rag_bm25_index* tl = ix->tail.get();
    *out = {ix->n_docs, ix->tail_docs, ix->nnz, tl ? tl->nnz : 0, bm_known_terms(ix), tl ? bm_segment_bytes(tl) : 0, ix->appends, ix->folds};
    return RAG_OK;
}
int bm25_segment_stats(rag_ctx* h, rag_bm25_segments* out) { return bm_segment_stats(h, bm_slot_bm25(h), out); }
int sparse_segment_stats(rag_ctx* h, rag_bm25_segments* out) { return bm_segment_stats(h, bm_slot_sparse(h), out); }

static int bm25_set_attr(rag_ctx* h) {
    return raise_lds(h, h->attr_bm25_lds, BM_LDS_BYTES, bm25_range_kernel<0, false>, bm25_range_kernel<0, true>, bm25_range_kernel<1, false>,
                     bm25_range_kernel<1, true>, bm25_range_kernel<2, false>, bm25_range_kernel<2, true>);
}

// The resident postings after rag_index_insert_host / rag_index_compact no longer describe the rows (the document count alone
// does not tell: i inserts then i compacted rows restore it): refuse until rag_bm25_append_host covers the inserted rows or
// rag_bm25_load_host reloads them (rag_index_compact_bm25 renumbers them with the rows and leaves this flag as it was).
// the two resident indexes of a handle (BM25 postings, learned-sparse postings) follow the dense index's rows when they cover them
static inline bool bm_resident(const rag_ctx* h, const rag_bm25_index* ix) { return ix == h->bm25 || ix == h->sparse; }
static int bm25_check_fresh(rag_ctx* h, const rag_bm25_index* ix) {
    if (ix == h->sparse && h->sparse_stale) {
        h->err = "sparse: the postings are stale (rows were inserted or compacted since rag_sparse_load_host): append the inserted "
                 "rows' postings (rag_sparse_append_host) or reload postings aligned with the current rows";
        return RAG_ERR_STATE;
    }
    if (ix != h->bm25 || !h->bm25_stale) return RAG_OK;
    h->err = "bm25: the postings are stale (rows were inserted or compacted since rag_bm25_load_host): reload postings aligned "
             "with the current rows";
    return RAG_ERR_STATE;
}

// the same check for the hybrid entry points, before their row-alignment checks (an insert changes the row count)
int bm25_fresh(rag_ctx* h) { return h->bm25 ? bm25_check_fresh(h, h->bm25) : RAG_OK; }

// doc ids follow the caller's id space when the postings cover exactly the index's rows (hybrid fusion needs one id space);
// any other postings - an ad-hoc index, a resident one beside an index of another size - report row numbers
static id_space bm_id_space(const rag_ctx* h, const rag_bm25_index* ix, id_space ids) {
    return bm_resident(h, ix) && h->n_rows == bm_total_docs(ix) ? ids : id_space::rows();
}

// common.h: loaded, fresh, row-aligned - with each entry's own code and text for missing postings
int keyword_postings_aligned(rag_ctx* h, bool sparse, const char* who, int missing_code, const char* note) {
    const rag_bm25_index* ix = sparse ? h->sparse : h->bm25;
    if (ix == nullptr && missing_code != RAG_OK) {          // (the texts are built on the refusing paths only: searches call this)
        h->err = std::string(missing_code == RAG_ERR_ARG ? "bad argument" : who) + ": no sparse index loaded (rag_sparse_load_host)";
        return missing_code;
    }
    if (int rc = ix ? bm25_check_fresh(h, ix) : RAG_OK) return rc;
    ARG_CHECK(h, ix != nullptr && bm_total_docs(ix) == h->n_rows,
              (std::string(who) + ": the " + (sparse ? "sparse" : "BM25") + " postings must be row-aligned with the index" + note).c_str());
    return RAG_OK;
}

// visibility argument of the scoring kernels (row_visible): the tenant filter and / or the deleted rows of the resident index
// (per-query tenants: some query is filtered, so the table is needed as under a scalar filter)
static int bm25_tenant_args(rag_ctx* h, const rag_bm25_index* ix, int tenant, query_tenants qt, const int32_t** tenants_out) {
    *tenants_out = nullptr;
    if (qt.host != nullptr) tenant = 0;
    if (int rc = bm25_check_fresh(h, ix)) return rc;
    if (tenant < 0) {
        if (bm_resident(h, ix) && h->vis != nullptr && h->n_rows == bm_total_docs(ix)) *tenants_out = h->vis;
        return RAG_OK;
    }
    ARG_CHECK(h, h->tenants != nullptr && h->n_rows == bm_total_docs(ix),
              "bm25: a tenant filter needs rag_index_set_tenants_host and postings row-aligned with the index");
    *tenants_out = search_vis(h, tenant);
    return RAG_OK;
}

// ---- statistics refresh (rag_bm25_live_counts_host / rag_bm25_set_statistics_host / rag_bm25_refresh) --------------------------
// Fresh idf / avgdl computed from, and written into, the resident postings (option bm25_keep_tf at load time). COUNT: document
// frequencies over the live postings, live documents, the sum of their lengths - all exact integers, so the atomics' order cannot
// show. RULE: rank-bm25's idf on the host (libm's log in float64: the table must be the bits Python's math.log gives). INSTALL: every
// impact of base and tail recomputed from (tf, doc_len, idf, avgdl) by the load's own arithmetic (bm_tf_factor), the packed
// base's table by bm25_gtab_kernel; offsets, bracket tables and the postings' order are not touched.

// live document frequencies of one segment, added into df[]: a workgroup takes a tile of BM_CP_TILE consecutive postings (the
// compaction's tiling), one ballot per 64 postings gives the tile's live mask in LDS, and every term that has postings in the
// tile - a tile is term-major, so these are the terms t_first .. t_last - counts the set bits of its own stretch: ONE atomic
// per (tile, term), none per posting.
__global__ __launch_bounds__(256) void bm25_live_df_kernel(const bm_term_meta* __restrict__ meta, int64_t n_terms, const int32_t* __restrict__ doc,
                                                            int64_t nnz, const int32_t* __restrict__ vis, int64_t row0, int32_t* __restrict__ df) {
    __shared__ unsigned long long mw[BM_CP_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * BM_CP_TILE, pe = min(p0 + BM_CP_TILE, nnz);
#pragma unroll
    for (int j = 0; j < BM_CP_TILE / 256; ++j) {
        const int64_t p = p0 + j * 256 + tid;
        const bool live = p < nnz && row_visible(vis, row0 + doc[p], -1);
        const unsigned long long m = __ballot(live);
        if (lane == 0) mw[j * 4 + wv] = m;
    }
    __syncthreads();
    const bm_term_by_meta term_of{meta, n_terms};
    const int64_t t_first = term_of(p0), t_last = term_of(pe - 1);
    for (int64_t t = t_first + tid; t <= t_last; t += 256) {
        const bm_term_meta m = meta[t];
        const int a = (int)(max(m.post, p0) - p0), e = (int)(min(m.post + m.df, pe) - p0);
        if (e <= a) continue;                                       // a term without postings (in this tile)
        int c = 0;
        for (int k = a >> 6; k <= (e - 1) >> 6; ++k) {
            unsigned long long x = mw[k];
            if (k == a >> 6) x &= ~0ull << (a & 63);
            if (k == (e - 1) >> 6 && (e & 63)) x &= (1ull << (e & 63)) - 1ull;
            c += __popcll(x);
        }
        if (c) atomicAdd(&df[t], c);
    }
}

// live documents of one segment and the sum of their lengths, added into out2[0] / out2[1] (64-bit integer atomics, one pair
// per wave)
__global__ __launch_bounds__(256) void bm25_live_len_kernel(const int32_t* __restrict__ dl, int64_t first, int64_t n_docs, int64_t row0,
                                                             const int32_t* __restrict__ vis, unsigned long long* __restrict__ out2) {
    long long c = 0, s = 0;
    for (int64_t d = first + (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * 256)
        if (row_visible(vis, row0 + d, -1)) {
            ++c;
            s += dl[d];
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o);
        s += __shfl_xor(s, o);
    }
    if ((threadIdx.x & 63) == 0 && c) {
        atomicAdd(&out2[0], (unsigned long long)c);
        atomicAdd(&out2[1], (unsigned long long)s);
    }
}

__global__ void bm25_set_idf_kernel(bm_term_meta* __restrict__ meta, int64_t n_terms, const double* __restrict__ idf) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_terms) meta[t].idf = idf[t];
}

static int bm25_refresh_ready(rag_ctx* h, const char* what) {
    if (!h->bm25) {
        h->err = std::string(what) + ": no postings loaded";
        return RAG_ERR_STATE;
    }
    if (!h->bm25->keep_tf) {
        h->err = std::string(what) + ": the postings were loaded without option bm25_keep_tf (term frequencies and document lengths were not kept)";
        return RAG_ERR_STATE;
    }
    return bm25_check_fresh(h, h->bm25);
}

// a document is live when it is covered and not deleted: the deleted rows of a row-aligned dense index, nobody otherwise
static const int32_t* bm_live_vis(const rag_ctx* h, const rag_bm25_index* ix) {
    return h->vis != nullptr && h->index_loaded && h->n_rows == bm_total_docs(ix) ? h->vis.get() : nullptr;
}

// the scratch of a refresh: 12 B per term + the two counters, all allocated before anything is overwritten
struct bm_refresh_ws {
    dev_buf<int32_t> df;
    dev_buf<double> idf;
    dev_buf<unsigned long long> cnt;
};

// COUNT. df_h[V] = live postings per term (base and tail together). Nothing deleted: the offsets' differences, no posting read.
static int bm25_count_live(rag_ctx* h, bm_refresh_ws& ws, std::vector<int32_t>& df_h, int64_t* n_live, int64_t* sum_dl) {
    const rag_bm25_index* ix = h->bm25;
    const rag_bm25_index* tl = ix->tail.get();
    const int64_t V = (int64_t)ix->idf_h.size();
    const int32_t* vis = bm_live_vis(h, ix);
    hipStream_t st = h->stream;
    df_h.assign((size_t)V, 0);
    unsigned long long cnt_h[2] = {0, 0};
    HIP_TRY(h, hipMemsetAsync(ws.cnt, 0, 2 * sizeof(unsigned long long), st));
    for (const rag_bm25_index* sg : {ix, tl}) {
        if (sg == nullptr) continue;
        const int64_t own = sg->n_docs - sg->first;
        if (own > 0)
            hipLaunchKernelGGL(bm25_live_len_kernel, dim3((unsigned)std::min<int64_t>(1024, (own + 255) / 256)), dim3(256), 0, st, sg->dl.get(),
                               (int64_t)sg->first, sg->n_docs, sg->row0, vis, ws.cnt.get());
    }
    if (vis != nullptr) {
        if (V) HIP_TRY(h, hipMemsetAsync(ws.df, 0, (size_t)V * sizeof(int32_t), st));
        for (const rag_bm25_index* sg : {ix, tl}) {
            if (sg == nullptr || sg->nnz == 0) continue;
            hipLaunchKernelGGL(bm25_live_df_kernel, dim3((unsigned)((sg->nnz + BM_CP_TILE - 1) / BM_CP_TILE)), dim3(256), 0, st, sg->meta.get(),
                               sg->n_terms, sg->doc.get(), sg->nnz, vis, sg->row0, ws.df.get());
        }
        if (V) HIP_TRY(h, hipMemcpyAsync(df_h.data(), ws.df, (size_t)V * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else {
        for (const rag_bm25_index* sg : {ix, tl}) {
            if (sg == nullptr) continue;
            for (int64_t t = 0; t < sg->n_terms; ++t) df_h[(size_t)t] += (int32_t)(sg->indptr_h[(size_t)t + 1] - sg->indptr_h[(size_t)t]);
        }
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(cnt_h, ws.cnt, sizeof(cnt_h), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    *n_live = (int64_t)cnt_h[0];
    *sum_dl = (int64_t)cnt_h[1];
    return RAG_OK;
}

// INSTALL. idf[V] (host) and avgdl become the statistics of base and tail.
static int bm25_install(rag_ctx* h, bm_refresh_ws& ws, const double* idf, double avgdl) {
    rag_bm25_index* ix = h->bm25;
    rag_bm25_index* tl = ix->tail.get();
    const int64_t V = (int64_t)ix->idf_h.size();
    hipStream_t st = h->stream;
    if (V) HIP_TRY(h, hipMemcpyAsync(ws.idf, idf, (size_t)V * sizeof(double), hipMemcpyHostToDevice, st));
    for (rag_bm25_index* sg : {ix, tl}) {
        if (sg == nullptr) continue;
        if (sg->packed != nullptr)
            bm_launch_1d(bm25_gtab_kernel, sg->n_codes, st, sg->tfv, sg->dlv, sg->n_codes, sg->n_dl, avgdl, sg->k1, sg->b, sg->gtab);
        else if (sg->nnz)                    // every impact again from the KEPT planes: one streaming pass of the load's own kernel
            bm_launch_1d(bm25_impact_kernel<uint16_t, bm_term_by_meta>, sg->nnz, st, bm_term_by_meta{sg->meta, sg->n_terms}, sg->doc, sg->tf16,
                         sg->dl, sg->nnz, avgdl, sg->k1, sg->b, ws.idf, sg->w);
        if (sg->n_terms) bm_launch_1d(bm25_set_idf_kernel, sg->n_terms, st, sg->meta, sg->n_terms, ws.idf);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(st));
    ix->idf_h.assign(idf, idf + V);
    ix->avgdl = avgdl;
    if (tl) tl->avgdl = avgdl;
    // recomputed, not kept: epsilon * mean can itself be negative on a tiny corpus (bm25_negative_bound_args)
    ix->neg_idf_absmax = 0.0;
    for (int64_t t = 0; t < V; ++t)
        if (idf[t] < 0.0) ix->neg_idf_absmax = std::max(ix->neg_idf_absmax, -idf[t]);
    return RAG_OK;
}

static int bm25_refresh_alloc(rag_ctx* h, bm_refresh_ws& ws, bool count, bool install, const char* what) {
    const size_t V = h->bm25->idf_h.size();
    int rc;
    if (count && (rc = bm_alloc(h, ws.df, V, what))) return rc;
    if (count && (rc = bm_alloc(h, ws.cnt, 2, what))) return rc;
    if (install && (rc = bm_alloc(h, ws.idf, V, what))) return rc;
    return RAG_OK;
}

int bm25_live_counts_host(rag_ctx* h, int32_t* df_out, int64_t* n_docs_live_out, int64_t* sum_doc_len_out) {
    const char* what = "bm25_live_counts";
    int rc = bm25_refresh_ready(h, what);
    if (rc) return rc;
    bm_refresh_ws ws;
    if ((rc = bm25_refresh_alloc(h, ws, true, false, what))) return rc;
    std::vector<int32_t> df_h;
    int64_t n_live = 0, sum_dl = 0;
    if ((rc = bm25_count_live(h, ws, df_h, &n_live, &sum_dl))) return rc;
    if (df_out && !df_h.empty()) memcpy(df_out, df_h.data(), df_h.size() * sizeof(int32_t));
    if (n_docs_live_out) *n_docs_live_out = n_live;
    if (sum_doc_len_out) *sum_doc_len_out = sum_dl;
    return RAG_OK;
}

static int bm25_check_statistics(rag_ctx* h, const double* idf, int64_t V, double avgdl, const char* what) {
    ARG_CHECK(h, V == 0 || idf != nullptr, "bm25_set_statistics: null idf table");
    ARG_CHECK(h, std::isfinite(avgdl) && avgdl > 0.0, "bm25_set_statistics: avgdl must be finite and > 0");
    for (int64_t t = 0; t < V; ++t) ARG_CHECK(h, std::isfinite(idf[t]), "bm25_set_statistics: every idf must be finite");
    return RAG_OK;
}

int bm25_set_statistics_host(rag_ctx* h, const double* idf, double avgdl) {
    const char* what = "bm25_set_statistics";
    int rc = bm25_refresh_ready(h, what);
    if (rc) return rc;
    if ((rc = bm25_check_statistics(h, idf, (int64_t)h->bm25->idf_h.size(), avgdl, what))) return rc;
    bm_refresh_ws ws;
    if ((rc = bm25_refresh_alloc(h, ws, false, true, what))) return rc;
    return bm25_install(h, ws, idf, avgdl);
}

int bm25_refresh(rag_ctx* h, double epsilon, double* idf_out, rag_bm25_refresh_info* info_out) {
    const char* what = "bm25_refresh";
    int rc = bm25_refresh_ready(h, what);
    if (rc) return rc;
    ARG_CHECK(h, std::isfinite(epsilon), "bm25_refresh: epsilon must be finite");
    rag_bm25_index* ix = h->bm25;
    const int64_t V = (int64_t)ix->idf_h.size();
    bm_refresh_ws ws;
    if ((rc = bm25_refresh_alloc(h, ws, true, true, what))) return rc;
    std::vector<int32_t> df;
    int64_t N = 0, sum_dl = 0;
    if ((rc = bm25_count_live(h, ws, df, &N, &sum_dl))) return rc;
    if (N <= 0) {
        h->err = "bm25_refresh: no live covered document remains";
        return RAG_ERR_STATE;
    }
    // rank-bm25's rule over the terms that still occur, in term-number order (= its dict order); float64, libm's log
    std::vector<double> idf((size_t)V);
    rag_bm25_refresh_info info = {};
    double sum = 0.0;
    int64_t occurring = 0;
    for (int64_t t = 0; t < V; ++t) {
        const int64_t d = df[(size_t)t];
        info.nnz_live += d;
        if (d == 0) {                        // lost every posting: stays in the vocabulary, out of the mean
            idf[(size_t)t] = std::log((double)N + 0.5) - std::log(0.5);
            info.terms_without_postings++;
            continue;
        }
        const double v = std::log((double)(N - d) + 0.5) - std::log((double)d + 0.5);
        idf[(size_t)t] = v;
        sum += v;
        occurring++;
    }
    const double mean = occurring ? sum / (double)occurring : 0.0;
    for (int64_t t = 0; t < V; ++t)
        if (df[(size_t)t] != 0 && idf[(size_t)t] < 0.0) {
            idf[(size_t)t] = epsilon * mean;
            info.negative_idf_terms++;
        }
    const double avgdl = (double)sum_dl / (double)N;
    if ((rc = bm25_check_statistics(h, idf.data(), V, avgdl, what))) return rc;     // (a corpus of empty documents: avgdl 0)
    info.n_docs_live = N;
    info.n_terms = V;
    info.avgdl_before = ix->avgdl;
    info.avgdl_after = avgdl;
    for (int64_t t = 0; t < V; ++t) info.idf_max_abs_change = std::max(info.idf_max_abs_change, std::fabs(idf[(size_t)t] - ix->idf_h[(size_t)t]));
    if ((rc = bm25_install(h, ws, idf.data(), avgdl))) return rc;
    if (idf_out && V) memcpy(idf_out, idf.data(), (size_t)V * sizeof(double));
    if (info_out) *info_out = info;
    return RAG_OK;
}

// ---- the per-call workspace of a keyword search: every plane named ONCE, in the order the buffer holds them (ws_carve: one pass
// sizes, one carves). mode 0: the partial lists [Q][ranges of both segments][k] with their counts, the running list, the threshold;
// both modes: the plan of both segments (the metadata sized for the largest plan_t). hw - the host entry, which stages everything
// in the handle's arena: additionally the query arrays (n_tok tokens), the outputs, the all-document plane of mode 1 and, for a
// call that has them, the query weights.
struct bm25_host_ws { int32_t* term_ptr; int32_t* terms; int64_t* ids; int32_t* rows; double* raw_max; double* scores; double* dense; float* qweights; };
static void bm25_ws_planes(ws_carve& c, const rag_bm25_index* ix, int Q, int k, int mode, int plan_t, bm25_topk_ws& w, bm25_host_ws* hw = nullptr,
                           size_t n_tok = 0, bool qweights = false) {
    const size_t nq = (size_t)Q, n_cnt = nq * bm_total_ranges(ix), n_part = mode == 0 ? n_cnt * k : 0, n_out = mode == 0 ? nq * k : 0;
    if (hw) hw->term_ptr = c.take<int32_t>(nq + 1);
    if (hw) hw->terms = c.take<int32_t>(n_tok);
    w.part_key = c.take<uint64_t>(n_part);
    w.part_row = c.take<uint32_t>(n_part);
    w.part_cnt = c.take<int>(n_cnt);
    w.run_key = c.take<uint64_t>(n_out);
    w.run_row = c.take<uint32_t>(n_out);
    w.tau = c.take<uint64_t>(nq);
    if (hw) {
        hw->ids = c.take<int64_t>(n_out);
        hw->rows = c.take<int32_t>(n_out);
        hw->raw_max = c.take<double>(nq);
        hw->scores = c.take<double>(n_out);
        hw->dense = c.take<double>(mode == 1 ? nq * bm_total_docs(ix) : 0);
    }
    w.plan.off = c.take<int32_t>(bm25_plan_off_total(ix, Q, plan_t));
    w.plan.meta = c.take<bm_plan_meta>(bm25_plan_meta_total(ix, Q));
    if (hw) hw->qweights = qweights ? c.take<float>(n_tok) : nullptr;
}
// What a query is BUDGETED at when a device call is cut into sub-batches (bm_topk_dev): per range its partial list (k x 12 B), the
// count and 8 plan slots x 4 B, plus the running list. It approximates the planes above - no 256-byte rounding, 8 slots whatever
// plan_t is, no plan metadata - and stays as it is: the number of sub-batches a budget gives is pinned by tests.
static size_t bm25_ws_per_query(const rag_bm25_index* ix, int k) {
    return (size_t)bm_total_ranges(ix) * ((size_t)k * 12 + 4 + 8 * 4) + (size_t)k * 12;
}
// the workspace of the device entry points, from the index's grow-only buffer
static int bm25_dev_ws(rag_ctx* h, rag_bm25_index* ix, int Q, int k, int mode, int plan_t, bm25_topk_ws& w) {
    ws_carve sum{nullptr};
    bm25_ws_planes(sum, ix, Q, k, mode, plan_t, w);
    if (int rc = ix->ws.reserve(h, sum.bytes)) return rc;
    ws_carve c{ix->ws};
    bm25_ws_planes(c, ix, Q, k, mode, plan_t, w);
    return RAG_OK;
}
static inline bool bm25_k_ok(int k) { return k > 0 && k <= BM_MERGE / 2 && k <= BM_RANGE; }

// host-pointer search against `ix` (the resident index or an ad-hoc one). Device staging comes from the handle's
// grow-only arena: no device allocation per call.
static int bm25_run(rag_ctx* h, const rag_bm25_index* ix, const int32_t* term_ptr, const int32_t* terms, int Q, int k, int mode, int tenant,
                    int64_t* ids_out, int32_t* rows_out, double* scores_out, double* raw_max_out, double* dense_out,
                    query_tenants qt = {nullptr, nullptr}, const float* qweights = nullptr) {
    ARG_CHECK(h, ix != nullptr, "no BM25 index loaded");
    ARG_CHECK(h, Q > 0 && Q <= 65535 && term_ptr, "bm25: 1 <= n_queries <= 65535");
    const int n_terms_q = term_ptr[Q];
    ARG_CHECK(h, n_terms_q >= 0 && (n_terms_q == 0 || terms), "bm25: bad term arrays");
    if (mode == 0) ARG_CHECK(h, bm25_k_ok(k), "bm25: 0 < k <= 1024");
    const int32_t* tenants = nullptr;
    hipStream_t st = h->stream;
    int rc;
    if ((rc = bm25_tenant_args(h, ix, mode == 0 ? tenant : -1, qt, &tenants))) return rc;
    if ((rc = bm25_set_attr(h))) return rc;
    int max_nt = 1;             // plan slots: the batch's longest query (term_ptr is on the host here), within the per-call budget
    for (int q = 0; q < Q; ++q) max_nt = std::max(max_nt, term_ptr[q + 1] - term_ptr[q]);
    const int plan_t = std::min(bm25_pick_plan_t(h, ix, Q), std::min(BM_PLAN_T, max_nt));
    bm25_topk_ws w;
    bm25_host_ws hw;
    ws_carve sum{nullptr};
    bm25_ws_planes(sum, ix, Q, k, mode, plan_t, w, &hw, std::max(1, n_terms_q), qweights != nullptr);
    if ((rc = stage_reserve(h, sum.bytes))) return rc;
    ws_carve c{h->stage};
    bm25_ws_planes(c, ix, Q, k, mode, plan_t, w, &hw, std::max(1, n_terms_q), qweights != nullptr);
    bm_range_call call = {ix, hw.term_ptr, hw.terms, hw.qweights, mode == 0 ? k : 1, mode, plan_t};
    call.tenants = tenants;                                            // (mode 1, bm25_scores_host: 0.0 for deleted rows)
    HIP_TRY(h, hipMemcpyAsync(hw.term_ptr, term_ptr, (size_t)(Q + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (n_terms_q) HIP_TRY(h, hipMemcpyAsync(hw.terms, terms, (size_t)n_terms_q * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (qweights && n_terms_q)                                         // the learned-sparse index: a weight per query token
        HIP_TRY(h, hipMemcpyAsync(hw.qweights, qweights, (size_t)n_terms_q * sizeof(float), hipMemcpyHostToDevice, st));
    if (mode == 0) {
        const size_t n_out = (size_t)Q * k;
        const id_space ids = bm_id_space(h, ix, id_space::of_index(h));       // a *_host search reports the index's ids
        const bm25_topk_out o = {ids.map, ids.base, hw.ids, hw.rows, hw.scores, hw.raw_max, ix->normalize};
        call.tenant = tenant;
        call.qten = qt.dev;
        bm25_launch_topk(h, call, Q, w, o, st);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(ids_out, hw.ids, n_out * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (rows_out) HIP_TRY(h, hipMemcpyAsync(rows_out, hw.rows, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(scores_out, hw.scores, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
        if (raw_max_out) HIP_TRY(h, hipMemcpyAsync(raw_max_out, hw.raw_max, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        call.dense_out = hw.dense;
        bm25_launch_scores(h, call, Q, w, st);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(dense_out, hw.dense, (size_t)Q * bm_total_docs(ix) * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    return RAG_OK;
}

// device-pointer entry: everything stays in HBM, asynchronous on `st` (workspace grows on first use / larger Q)
static int bm25_topk_dev_batch(rag_ctx* h, rag_bm25_index* ix, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                               int Q, int k, int tenant, int64_t* ids_dev, int32_t* rows_dev, double* scores_dev, double* raw_max_dev,
                               hipStream_t st, id_space ids, query_tenants qt) {
    ARG_CHECK(h, Q > 0 && Q <= 65535 && term_ptr_dev && ids_dev && scores_dev, "bm25_topk_dev: bad arguments");
    ARG_CHECK(h, bm25_k_ok(k), "bm25: 0 < k <= 1024");
    bm_range_call call = {ix, term_ptr_dev, terms_dev, qweights_dev, k, 0, bm25_pick_plan_t(h, ix, Q)};
    call.tenant = tenant;
    call.qten = qt.dev;
    int rc = bm25_tenant_args(h, ix, tenant, qt, &call.tenants);
    if (rc) return rc;
    if ((rc = bm25_set_attr(h))) return rc;
    bm25_topk_ws w;
    if ((rc = bm25_dev_ws(h, ix, Q, k, 0, call.plan_t, w))) return rc;
    ids = bm_id_space(h, ix, ids);
    const bm25_topk_out o = {ids.map, ids.base, ids_dev, rows_dev, scores_dev, raw_max_dev, ix->normalize};
    if ((rc = prof_begin(h, 1, st))) return rc;
    bm25_launch_topk(h, call, Q, w, o, st);
    HIP_TRY(h, hipGetLastError());
    return prof_end(h, 1, st);
}

// The per-call workspace (partial lists [Q][n_ranges][k] x 12 B + the plan) grows with Q x shard size: on a 12.5M-document shard a
// query takes ~9 MB at k = 100. Batches are therefore run in sub-batches whose workspace stays under BM_WS_BUDGET (queries are
// independent: same results; the 1M-document bench index runs 1,024 queries in one piece, the 12.5M-document shard 256).
#define BM_WS_BUDGET ((size_t)6 << 30)
// ix: the resident BM25 postings (bm25_topk_dev) or the learned-sparse postings (sparse_topk_dev, with the queries' weights)
static int bm_topk_dev(rag_ctx* h, rag_bm25_index* ix, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev, int Q,
                       int k, int tenant, int64_t* ids_dev, int32_t* rows_dev, double* scores_dev, double* raw_max_dev, hipStream_t st,
                       id_space ids, query_tenants qt) {
    ARG_CHECK(h, ix != nullptr, "no BM25 index loaded");
    ARG_CHECK(h, Q > 0 && Q <= 65535 && k > 0, "bm25_topk_dev: bad arguments");
    if (int rc = bm25_check_fresh(h, ix)) return rc;
    const size_t budget = h->opt.bm25_ws_mb > 0 ? (size_t)h->opt.bm25_ws_mb << 20 : BM_WS_BUDGET;
    const int qb = (int)std::max<size_t>(1, std::min<size_t>((size_t)Q, budget / std::max<size_t>(1, bm25_ws_per_query(ix, k))));
    for (int q0 = 0; q0 < Q; q0 += qb) {
        const int nq = std::min(qb, Q - q0);
        const int rc = bm25_topk_dev_batch(h, ix, term_ptr_dev + q0, terms_dev, qweights_dev, nq, k, tenant, ids_dev + (size_t)q0 * k,
                                           rows_dev ? rows_dev + (size_t)q0 * k : nullptr, scores_dev + (size_t)q0 * k,
                                           raw_max_dev ? raw_max_dev + q0 : nullptr, st, ids, qt + q0);      // (the tenants go with their queries)
        if (rc) return rc;
    }
    return RAG_OK;
}
int bm25_topk_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, int k, int tenant, int64_t* ids_dev,
                  int32_t* rows_dev, double* scores_dev, double* raw_max_dev, hipStream_t st, id_space ids, query_tenants qt) {
    return bm_topk_dev(h, h->bm25, term_ptr_dev, terms_dev, nullptr, Q, k, tenant, ids_dev, rows_dev, scores_dev, raw_max_dev, st, ids, qt);
}

// raw float64 scores of EVERY document for Q queries, device pointers, asynchronous: out_dev[Q][n_docs]
// (the all-document BM25Okapi.get_scores of rag/retrieval.py:340-341, for the index-level linear fusion)
// raw32_dev / ld / max_key_dev (all optional): see bm_dense_extra; `tenant` restricts the maximum to the tenant's documents
int bm25_scores_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, int Q, double* out_dev, hipStream_t st,
                    float* raw32_dev, int64_t ld, unsigned long long* max_key_dev, int tenant, query_tenants qt) {
    ARG_CHECK(h, h->bm25 != nullptr, "no BM25 index loaded");
    ARG_CHECK(h, Q > 0 && Q <= 65535 && term_ptr_dev && out_dev, "bm25_scores_dev: bad arguments");
    rag_bm25_index* ix = h->bm25;
    int rc = bm25_set_attr(h);
    if (rc) return rc;
    bm_range_call call = {ix, term_ptr_dev, terms_dev, nullptr, 1, 1, bm25_pick_plan_t(h, ix, Q)};
    call.tenant = tenant;
    call.qten = qt.dev;
    call.dense_out = out_dev;
    call.dx = {raw32_dev, ld, max_key_dev};
    if ((rc = bm25_check_fresh(h, ix))) return rc;
    if (max_key_dev != nullptr && (rc = bm25_tenant_args(h, ix, tenant, qt, &call.tenants))) return rc;
    bm25_topk_ws w;
    if ((rc = bm25_dev_ws(h, ix, Q, 1, 1, call.plan_t, w))) return rc;
    bm25_launch_scores(h, call, Q, w, st);
    HIP_TRY(h, hipGetLastError());
    return RAG_OK;
}

int bm25_set_normalize(rag_ctx* h, int on) {
    ARG_CHECK(h, h->bm25 != nullptr, "no BM25 index loaded");
    h->bm25->normalize = on ? 1 : 0;
    return RAG_OK;
}

int64_t bm25_n_docs(const rag_ctx* h) { return h->bm25 ? bm_total_docs(h->bm25) : -1; }

// What bounds a NEGATIVE raw score from the query alone (linear_scale_kernel, the fused emission margin): a raw score is a sum over
// the query's tokens of idf[t] * tf (k1+1) / (tf + k1 (1 - b + b dl / avgdl)), and the tf factor is at most k1 + 1 for k1 >= 0 and
// 0 <= b <= 1 (the denominator is then >= tf), so no score is below -(tokens of the query) * neg_idf_absmax * (k1 + 1).
// per_token_out = neg_idf_absmax * (k1 + 1): 0 when no idf is negative, +inf for parameters outside that range.
int bm25_negative_bound_args(const rag_ctx* h, double* per_token_out) {
    if (!h->bm25) return RAG_ERR_ARG;
    const rag_bm25_index* ix = h->bm25;
    const bool std_params = ix->k1 >= 0.0 && ix->b >= 0.0 && ix->b <= 1.0;
    *per_token_out = ix->neg_idf_absmax > 0.0 ? (std_params ? ix->neg_idf_absmax * (ix->k1 + 1.0) : (double)INFINITY) : 0.0;
    return RAG_OK;
}

// HBM bytes of an index built from these postings, from the host CSR offsets alone (no device call): postings (doc + impact,
// 12 B each), per-term metadata (32 B each) and the bracket tables (4 B per entry, <= nnz bytes by construction).
// launch geometry of one scoring launch (bm_make_grid), for tests and capacity planning: out = {workgroups, ranges, queries, query groups
// per range, queries per group (0: range-major order)}
int bm25_grid_plan(int n_ranges_in_launch, int n_queries, int linear, int64_t* out5) {
    if (!out5 || n_ranges_in_launch <= 0 || n_queries <= 0) return RAG_ERR_ARG;
    const bm_grid g = bm_make_grid(n_ranges_in_launch, n_queries, linear);
    out5[0] = g.blocks; out5[1] = g.nr_l; out5[2] = g.n_queries; out5[3] = g.n_groups; out5[4] = g.qgroup_len;
    return RAG_OK;
}

int bm25_index_bytes(const int64_t* indptr, int64_t n_docs, int64_t n_terms, int64_t* postings_out, int64_t* meta_out, int64_t* table_out) {
    if (!indptr || n_docs <= 0 || n_terms < 0) return RAG_ERR_ARG;
    const int64_t n_tab = bm_plan_terms(indptr, n_terms, n_docs, nullptr, INT64_MAX, nullptr);
    if (n_tab < 0) return RAG_ERR_ARG;
    if (postings_out) *postings_out = ((n_terms ? indptr[n_terms] - indptr[0] : 0) + 8) * 12;     // default form: doc i32 + impact f64
    if (meta_out) *meta_out = n_terms * (int64_t)sizeof(bm_term_meta);
    if (table_out) *table_out = n_tab * 4;
    return RAG_OK;
}

int bm25_topk_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, int Q, int k, int tenant, int64_t* ids_out,
                   int32_t* rows_out, double* scores_out, double* raw_max_out, query_tenants qt) {
    ARG_CHECK(h, ids_out && scores_out, "bm25_topk: null output");
    return bm25_run(h, h->bm25, term_ptr, terms, Q, k, 0, tenant, ids_out, rows_out, scores_out, raw_max_out, nullptr, qt);
}

int bm25_scores_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, int Q, double* out) {
    ARG_CHECK(h, out, "bm25_scores: null output");
    return bm25_run(h, h->bm25, term_ptr, terms, Q, 1, 1, -1, nullptr, nullptr, nullptr, nullptr, out);
}

// Stateless scoring of an AD-HOC corpus (HybridRetriever.hybrid_search builds a fresh BM25Okapi over the corpus it is handed on
// every call, rag/retrieval.py:333-341): the postings are uploaded, scored and dropped inside the call; the resident
// postings of the index (rag_bm25_load_host) are not touched.
int bm25_scores_adhoc_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const int32_t* tf, const int32_t* doc_len,
                           const double* idf, int64_t n_docs, int64_t n_terms, double avgdl, double k1, double b,
                           const int32_t* term_ptr, const int32_t* terms, int Q, double* out) {
    ARG_CHECK(h, out, "bm25_scores_adhoc: null output");
    std::unique_ptr<rag_bm25_index> ix;         // dropped when the call returns
    if (int rc = bm25_build(h, indptr, doc, tf, doc_len, idf, n_docs, n_terms, avgdl, k1, b, &ix)) return rc;
    return bm25_run(h, ix.get(), term_ptr, terms, Q, 1, 1, -1, nullptr, nullptr, nullptr, nullptr, out);
}

// ---- the learned-sparse inverted index (rag_sparse_*) ---------------------------------------------------------------------------
// A second resident index beside the BM25 postings, in its own slot (rag_ctx::sparse): term-major (doc i32, weight f32) postings of
// a learned-sparse model - bge-m3's lexical head, SPLADE, any {token id: weight} map - and queries whose tokens carry a float32
// weight. score(q, d) = sum over the query's tokens IN ORDER of (double)qw * (double)w[term, d], float64; the top-k holds only
// documents with score > 0. Everything but the posting form is the BM25 machinery above: metadata and bracket tables (idf = 1),
// the per-call plan (its float64 slot carries the query weight), staged thresholds, the merges, the visibility rules.
void sparse_free(rag_ctx* h) {
    delete h->sparse;
    h->sparse = nullptr;
}

int sparse_load_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const float* weight, int64_t n_docs, int64_t n_terms) {
    ARG_CHECK(h, n_docs >= 1 && n_terms >= 1 && n_docs < 0x7fffffff, "sparse_load: need n_docs >= 1 and n_terms >= 1");
    ARG_CHECK(h, indptr != nullptr && indptr[0] == 0, "sparse_load: indptr must start at 0");
    for (int64_t t = 0; t < n_terms; ++t)
        ARG_CHECK(h, indptr[t + 1] >= indptr[t] && indptr[t + 1] - indptr[t] <= n_docs,
                  "sparse_load: indptr must be non-decreasing with at most n_docs postings per term");
    const int64_t nnz = indptr[n_terms];
    ARG_CHECK(h, nnz == 0 || (doc && weight), "sparse_load: null postings");
    for (int64_t t = 0; t < n_terms; ++t)
        for (int64_t p = indptr[t]; p < indptr[t + 1]; ++p) {
            ARG_CHECK(h, doc[p] >= 0 && doc[p] < n_docs && (p == indptr[t] || doc[p] > doc[p - 1]),
                      "sparse_load: document numbers of a term must be strictly ascending and in [0, n_docs)");
            ARG_CHECK(h, std::isfinite(weight[p]) && weight[p] > 0.0f, "sparse_load: weights must be finite and > 0");
        }
    const bm_builder B = {h, "sparse_load", false};
    std::unique_ptr<rag_bm25_index> ix = bm_new_segment(nullptr, 0, n_docs, n_terms);
    ix->nnz = nnz;
    ix->indptr_h.assign(indptr, indptr + n_terms + 1);   // the fold and the compaction's remap plan from the host offsets
    ix->normalize = 0;                                   // scores are raw
    std::vector<bm_term_meta> meta_h;
    ix->tab_entries = bm_plan_terms(indptr, n_terms, n_docs, nullptr, n_docs, &meta_h);
    hipStream_t st = h->stream;
    auto enqueue = [&]() -> int {
        int rc;
        if ((rc = bm_prepare_segment(B, ix.get(), meta_h, {false, false, false, false, false, true}))) return rc;
        if (nnz) HIP_TRY(h, hipMemcpyAsync(ix->doc, doc, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (nnz) HIP_TRY(h, hipMemcpyAsync(ix->wf, weight, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, st));
        return RAG_OK;
    };
    if (int rc = bm_finish_segment(B, ix.get(), enqueue())) return rc;
    sparse_free(h);
    h->sparse = ix.release();
    h->sparse_stale = false;
    h->sparse_compacted = false;
    return RAG_OK;
}

// The next n_new rows behind the covered ones (rag_sparse_append_host): bm25_append_host's tail rebuild with the block's float32
// weights uploaded as they are. Everything is checked on the host before anything is built; a failure changes nothing.
int sparse_append_host(rag_ctx* h, const int64_t* indptr, const int32_t* doc, const float* weight, int64_t n_new, int64_t n_terms_total) {
    if (!h->sparse) {
        h->err = "sparse_append: no postings loaded (rag_sparse_load_host first)";
        return RAG_ERR_STATE;
    }
    const bm_slot S = bm_slot_sparse(h);
    rag_bm25_index* ix = h->sparse;
    const int64_t V = n_terms_total;
    if (int rc = bm_check_block(h, S.append_name, ix, indptr, doc, n_new, V, true, weight != nullptr)) return rc;
    const int64_t nnz_b = indptr[V];
    for (int64_t p = 0; p < nnz_b; ++p)
        ARG_CHECK(h, std::isfinite(weight[p]) && weight[p] > 0.0f, "sparse_append: weights must be finite and > 0");
    const bm_builder B = {h, S.append_name, true};
    dev_buf<float> b_w;
    auto fill = [&](const int64_t*, const int32_t*, const float** w_out, const uint16_t** tf16_out) -> int {
        if (int rc = bm_alloc(h, b_w, (size_t)nnz_b, B.what)) return rc;
        if (nnz_b) HIP_TRY(h, hipMemcpyAsync(b_w, weight, (size_t)nnz_b * sizeof(float), hipMemcpyHostToDevice, h->stream));
        *w_out = b_w;
        *tf16_out = nullptr;
        return RAG_OK;
    };
    std::unique_ptr<rag_bm25_index> nt;
    if (int rc = bm_build_tail<float>(h, B, ix, indptr, doc, nullptr, n_new, V, nullptr, fill, &nt)) return rc;
    bm_append_commit(h, S, std::move(nt), n_new);
    return RAG_OK;
}

// ---- a doc-major block on the device -> the term-major block an append takes (rag_sparse_append_dev) ---------------------------
// The block as rag_lexical_compact_dev writes it: doc_ptr int32 [n + 1] from 0, every document's terms ascending, float32 weights
// > 0. Its transpose - per-term lists, documents ascending inside a term - is what bm_build_tail concatenates behind the old tail.
//   1. sparse_docs_check_kernel: every fault a host append would refuse, and the per-term counts (integer atomics: any order
//      gives the same counts). The first fault - offsets before postings, then the lowest position - goes into one 64-bit word.
//   2. bm_scan_kernel: counts -> offsets. Offsets and the fault word come back in ONE copy (V + 2 int64); the host plans the
//      segment from them as it does from a host block's offsets. Nothing per posting crosses PCIe.
//   3. sparse_docs_expand_kernel: (term, document, weight) of every posting into private planes (later passes never read the
//      caller's arrays again), then a STABLE least-significant-digit counting sort over the term number, BM_TR_BITS bits a pass:
//      per-tile digit counts, one scan over (digit, tile), and a scatter that ranks a posting among the tile's earlier postings
//      of its digit. The block comes in document order, so stability alone leaves every term's documents ascending: the
//      permutation is np.argsort(term * n + document, kind="stable"), whatever the launch order. No grid depends on V and a
//      term in every document is spread over tiles like any other.
#define BM_TR_BITS 6
#define BM_TR_BUCKETS (1 << BM_TR_BITS)
#define BM_TR_TILE 2048
#define BM_TR_THREADS 256
#define BM_TR_WAVES (BM_TR_THREADS / 64)
static_assert(BM_TR_BUCKETS == 64, "the scatter ranks one digit per lane of a wave");
// digit passes that order term numbers below V
static inline int bm_tr_passes(int64_t V) {
    int passes = 0;
    for (int64_t m = V - 1; m > 0; m >>= BM_TR_BITS) ++passes;
    return passes;
}

// the fault word: class (0 an offset, 1 a posting) << 60 | position << 4 | code; the smallest wins, BM_TR_NO_FAULT: none
#define BM_TR_NO_FAULT (~0ull)
static const char* const bm_tr_fault_text[] = {
    "",
    "doc_ptr must start at 0",
    "doc_ptr must never decrease",
    "doc_ptr ends past nnz_cap (the block was cut at its capacity)",
    "term outside [0, n_terms_total)",
    "terms must be strictly ascending inside a document",
    "weights must be finite and > 0",
};

// owner of posting p: the last document whose offset is <= p (bm_last_le's empty-list rule); in [0, n) for ANY offsets
__device__ __forceinline__ int64_t bm_tr_doc_of(const int32_t* __restrict__ doc_ptr, int64_t n, int64_t p) {
    return bm_last_le(n, p, [&](int64_t d) { return (int64_t)doc_ptr[d]; });
}
// postings the kernels may touch: doc_ptr[n] clamped to the arrays' capacity, so no read depends on the block being well formed
__device__ __forceinline__ int64_t bm_tr_nnz(const int32_t* __restrict__ doc_ptr, int64_t n, int64_t nnz_cap) {
    return std::min<int64_t>(std::max<int64_t>(doc_ptr[n], 0), nnz_cap);
}

// one thread per offset AND per posting slot (grid over max(n + 1, nnz_cap))
__global__ __launch_bounds__(256) void sparse_docs_check_kernel(const int32_t* __restrict__ doc_ptr, const int32_t* __restrict__ terms,
                                                                const float* __restrict__ weights, int64_t n, int64_t nnz_cap, int64_t V,
                                                                uint32_t* __restrict__ count, unsigned long long* __restrict__ fault) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = BM_TR_NO_FAULT;
    if (p <= n) {
        int code = 0;
        if (p == 0 && doc_ptr[0] != 0) code = 1;
        else if (p < n && doc_ptr[p + 1] < doc_ptr[p]) code = 2;
        else if (p == n && doc_ptr[n] > nnz_cap) code = 3;
        if (code) bad = ((unsigned long long)p << 4) | (unsigned)code;
    }
    if (p < bm_tr_nnz(doc_ptr, n, nnz_cap)) {
        const int64_t d = bm_tr_doc_of(doc_ptr, n, p);
        const int32_t t = terms[p];
        const float w = weights[p];
        int code = 0;
        if (t < 0 || t >= V) code = 4;
        else if (p > 0 && p > doc_ptr[d] && terms[p - 1] >= t) code = 5;      // (p > 0: a NEGATIVE offset may not send the look-back before the array)
        else if (!(__builtin_isfinite(w) && w > 0.0f)) code = 6;
        if (code) bad = std::min(bad, (1ull << 60) | ((unsigned long long)p << 4) | (unsigned)code);
        if (code != 4) atomicAdd(&count[t], 1u);
    }
    if (bad != BM_TR_NO_FAULT) atomicMin(fault, bad);
}

// out[i] = count[0] + .. + count[i - 1] for i in [0, n]: ONE workgroup, a contiguous stretch per thread. Sized for what an
// ingest brings: V counts (250,002 for bge-m3) and nnz / 32 per-(digit, tile) counts - 2,500 for a 1,000-text block, about
// 250,000 (the size of the V scan) for the 8 M postings of 65,535 texts. Up to there the scans are small beside the passes.
// They stay correct to the call's limit of 2^31 postings but are not built for it: 67 M counts, 268 MB, would go through one
// workgroup three times, no longer small beside the passes; a block of that size wants a scan over many workgroups first.
template <class O>
__global__ __launch_bounds__(1024) void bm_scan_kernel(const uint32_t* __restrict__ count, int64_t n, O* __restrict__ out) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = std::min<int64_t>(tid * per, n), hi = std::min<int64_t>(lo + per, n);
    int64_t own = 0;
    for (int64_t i = lo; i < hi; ++i) own += count[i];
    part[tid] = own;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t below = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += below;
        __syncthreads();
    }
    int64_t run = part[tid] - own;
    for (int64_t i = lo; i < hi; ++i) {
        out[i] = (O)run;
        run += count[i];
    }
    if (tid == 1023) out[n] = (O)part[1023];
}

__global__ __launch_bounds__(256) void sparse_docs_expand_kernel(const int32_t* __restrict__ doc_ptr, const int32_t* __restrict__ terms,
                                                                 const float* __restrict__ weights, int64_t n, int64_t nnz,
                                                                 int32_t* __restrict__ key_out, int32_t* __restrict__ doc_out,
                                                                 float* __restrict__ w_out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    key_out[p] = terms[p];
    doc_out[p] = (int32_t)bm_tr_doc_of(doc_ptr, n, p);
    w_out[p] = weights[p];
}

// digit counts of one tile of BM_TR_TILE consecutive postings, stored digit-major: tile_count[digit * n_tiles + tile]
__global__ __launch_bounds__(BM_TR_THREADS) void bm_tr_count_kernel(const int32_t* __restrict__ key, int64_t nnz, int shift, int64_t n_tiles,
                                                                    uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t cnt[BM_TR_BUCKETS];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x, p0 = tile * BM_TR_TILE;
    if (tid < BM_TR_BUCKETS) cnt[tid] = 0;
    __syncthreads();
    for (int i = tid; i < BM_TR_TILE && p0 + i < nnz; i += BM_TR_THREADS) atomicAdd(&cnt[(key[p0 + i] >> shift) & (BM_TR_BUCKETS - 1)], 1u);
    __syncthreads();
    if (tid < BM_TR_BUCKETS) tile_count[(int64_t)tid * n_tiles + tile] = cnt[tid];
}

// The stable scatter of one tile. tile_off = the scan of tile_count: where the tile's first posting of each digit goes. The tile
// is walked in rounds of one posting per thread; inside a round a posting's rank among the earlier ones of its digit is the
// round's earlier waves' counts plus the lower lanes of its own wave with the same digit (six ballots).
__global__ __launch_bounds__(BM_TR_THREADS) void bm_tr_scatter_kernel(const int32_t* __restrict__ key, const int32_t* __restrict__ doc,
                                                                      const float* __restrict__ w, int64_t nnz, int shift, int64_t n_tiles,
                                                                      const uint32_t* __restrict__ tile_off, int32_t* __restrict__ key_out,
                                                                      int32_t* __restrict__ doc_out, float* __restrict__ w_out) {
    __shared__ uint32_t base[BM_TR_BUCKETS];
    __shared__ uint32_t wave_cnt[BM_TR_WAVES][BM_TR_BUCKETS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t tile = blockIdx.x, p0 = tile * BM_TR_TILE;
    if (tid < BM_TR_BUCKETS) base[tid] = tile_off[(int64_t)tid * n_tiles + tile];
    wave_cnt[wv][lane] = 0;
    __syncthreads();
    for (int r = 0; r < BM_TR_TILE / BM_TR_THREADS && p0 + r * BM_TR_THREADS < nnz; ++r) {      // (uniform bounds: every thread meets every barrier)
        const int64_t p = p0 + r * BM_TR_THREADS + tid;
        const bool valid = p < nnz;
        const int32_t k = valid ? key[p] : 0;
        const int dg = (k >> shift) & (BM_TR_BUCKETS - 1);
        uint64_t same = __ballot(valid);
        for (int b = 0; b < BM_TR_BITS; ++b) {
            const bool bit = (dg >> b) & 1;
            const uint64_t bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wave_cnt[wv][dg] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t o = base[dg] + (uint32_t)rank;
            for (int x = 0; x < wv; ++x) o += wave_cnt[x][dg];
            if ((int64_t)o < nnz) {          // always, when counts and keys agree: kept so that no input can send a store outside
                key_out[o] = k;
                doc_out[o] = doc[p];
                w_out[o] = w[p];
            }
        }
        __syncthreads();
        if (tid < BM_TR_BUCKETS)
            for (int x = 0; x < BM_TR_WAVES; ++x) {
                base[tid] += wave_cnt[x][tid];
                wave_cnt[x][tid] = 0;
            }
        __syncthreads();
    }
}

// The transposed block on the device and what the host needs of it. The planes live as long as this object: TWO allocations,
// the offsets (with the per-term counts behind them) before the one synchronise and the sort's planes after it.
struct bm_term_block {
    std::vector<int64_t> indptr_h;           // [V + 2]: the offsets, then the fault word
    dev_buf<int64_t> indptr;                 // the same on the device, then uint32 count[V]
    dev_buf<int32_t> planes;                 // key / doc / weight of both sides of the sort, tile_count, tile_off: 4-byte words
    const int32_t* b_doc = nullptr;
    const float* b_w = nullptr;
    int64_t nnz = 0;
};

// Validates and transposes on the handle's stream; synchronises once for the offsets. RAG_ERR_ARG names the first fault.
static int sparse_transpose_docs(rag_ctx* h, const char* who, const int32_t* doc_ptr, const int32_t* terms, const float* weights, int64_t n,
                                 int64_t nnz_cap, int64_t V, bm_term_block& T) {
    hipStream_t st = h->stream;
    int rc;
    if ((rc = bm_alloc(h, T.indptr, (size_t)V + 2 + ((size_t)V + 1) / 2, who))) return rc;
    uint32_t* count = reinterpret_cast<uint32_t*>(T.indptr + V + 2);
    try {
        T.indptr_h.resize((size_t)V + 2);
    } catch (const std::bad_alloc&) {
        h->err = std::string(who) + ": out of host memory";
        return RAG_ERR_NOMEM;
    }
    HIP_TRY(h, hipMemsetAsync(count, 0, (size_t)V * sizeof(uint32_t), st));
    HIP_TRY(h, hipMemsetAsync(T.indptr + V + 1, 0xff, sizeof(int64_t), st));
    bm_launch_1d(sparse_docs_check_kernel, std::max(n + 1, nnz_cap), st, doc_ptr, terms, weights, n, nnz_cap, V, count,
                 reinterpret_cast<unsigned long long*>(T.indptr + V + 1));
    hipLaunchKernelGGL(bm_scan_kernel<int64_t>, dim3(1), dim3(1024), 0, st, count, V, T.indptr.get());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(T.indptr_h.data(), T.indptr, (size_t)(V + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const unsigned long long fault = (unsigned long long)T.indptr_h[(size_t)V + 1];
    if (fault != BM_TR_NO_FAULT) {
        const int code = (int)(fault & 15);
        const long long pos = (long long)((fault >> 4) & 0xffffffffffull);
        ARG_CHECK(h, false, std::string(who) + ": " + bm_tr_fault_text[code] + " (" + ((fault >> 60) ? "posting " : "document ") + std::to_string(pos) + ")");
    }
    const int64_t nnz = T.nnz = T.indptr_h[(size_t)V];
    const int passes = nnz ? bm_tr_passes(V) : 0;                    // (a block of empty documents sorts nothing)
    const int64_t n_tiles = (nnz + BM_TR_TILE - 1) / BM_TR_TILE, n_cnt = n_tiles * BM_TR_BUCKETS;
    // one plane set when no pass runs, two to sort between; the tile tables behind them
    if ((rc = bm_alloc(h, T.planes, (size_t)(3 * nnz * (passes ? 2 : 1) + (passes ? 2 * n_cnt + 1 : 0)), who))) return rc;
    int32_t* key[2] = {T.planes.get(), T.planes + 3 * nnz};
    int32_t* docp[2] = {key[0] + nnz, key[1] + nnz};
    float* wp[2] = {reinterpret_cast<float*>(key[0] + 2 * nnz), reinterpret_cast<float*>(key[1] + 2 * nnz)};
    uint32_t* tile_count = reinterpret_cast<uint32_t*>(T.planes + 6 * nnz);
    uint32_t* tile_off = tile_count + n_cnt;
    int cur = 0;
    if (nnz) {
        bm_launch_1d(sparse_docs_expand_kernel, nnz, st, doc_ptr, terms, weights, n, nnz, key[0], docp[0], wp[0]);
        for (int pass = 0; pass < passes; ++pass, cur ^= 1) {
            const int shift = pass * BM_TR_BITS;
            hipLaunchKernelGGL(bm_tr_count_kernel, dim3((unsigned)n_tiles), dim3(BM_TR_THREADS), 0, st, key[cur], nnz, shift, n_tiles, tile_count);
            hipLaunchKernelGGL(bm_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, tile_count, n_cnt, tile_off);
            hipLaunchKernelGGL(bm_tr_scatter_kernel, dim3((unsigned)n_tiles), dim3(BM_TR_THREADS), 0, st, key[cur], docp[cur], wp[cur], nnz, shift,
                               n_tiles, tile_off, key[cur ^ 1], docp[cur ^ 1], wp[cur ^ 1]);
        }
        HIP_TRY(h, hipGetLastError());
    }
    T.b_doc = docp[cur];
    T.b_w = wp[cur];
    return RAG_OK;
}

// rag_sparse_append_dev: the next n rows from a doc-major device block. With postings resident it is sparse_append_host of the
// transposed block (the same bm_build_tail, the block's planes already on the device); without, the block becomes the base as
// sparse_load_host builds it. Nothing resident is touched before everything has been built.
int sparse_append_docs_dev(rag_ctx* h, const int32_t* doc_ptr, const int32_t* terms, const float* weights, int64_t n, int64_t nnz_cap,
                           int64_t n_terms_total) {
    const bm_slot S = bm_slot_sparse(h);
    rag_bm25_index* ix = h->sparse;
    const std::string w = std::string(S.append_name) + ": ";
    const int64_t V = n_terms_total, known = ix ? bm_known_terms(ix) : 0, covered = ix ? bm_total_docs(ix) : 0;
    ARG_CHECK(h, n >= 1 && covered + n < 0x7fffffff, w + "n_docs_new must be >= 1 (and the index stay under 2^31 documents)");
    ARG_CHECK(h, V >= 1 && V >= known && V < 0x7fffffff, w + "n_terms_total may not shrink");
    ARG_CHECK(h, nnz_cap >= 0 && nnz_cap <= 0x7fffffff, w + "nnz_cap must lie in [0, 2^31)");
    ARG_CHECK(h, doc_ptr && (nnz_cap == 0 || (terms && weights)), w + "null pointer");
    ARG_CHECK(h, !h->index_loaded || covered + n <= h->n_rows, w + "the block would cover more rows than the index has");
    const bm_builder B = {h, S.append_name, true};
    bm_term_block T;
    if (int rc = sparse_transpose_docs(h, B.what, doc_ptr, terms, weights, n, nnz_cap, V, T)) {
        (void)hipStreamSynchronize(h->stream);          // T's planes are freed on return
        return rc;
    }
    if (ix != nullptr) {
        auto fill = [&](const int64_t*, const int32_t*, const float** w_out, const uint16_t** tf16_out) -> int {
            *w_out = T.b_w;
            *tf16_out = nullptr;
            return RAG_OK;
        };
        std::unique_ptr<rag_bm25_index> nt;
        if (int rc = bm_build_tail<float>(h, B, ix, T.indptr_h.data(), nullptr, nullptr, n, V, nullptr, fill, &nt, T.indptr.get(), T.b_doc)) return rc;
        bm_append_commit(h, S, std::move(nt), n);
        return RAG_OK;
    }
    std::unique_ptr<rag_bm25_index> nb = bm_new_segment(nullptr, 0, n, V);
    nb->indptr_h.assign(T.indptr_h.begin(), T.indptr_h.begin() + V + 1);
    nb->normalize = 0;
    std::vector<bm_term_meta> meta_h;
    bm_plan_segment(nb.get(), nullptr, meta_h);
    hipStream_t st = h->stream;
    auto enqueue = [&]() -> int {
        if (int rc = bm_prepare_segment(B, nb.get(), meta_h, {false, false, false, false, false, true})) return rc;
        if (T.nnz) HIP_TRY(h, hipMemcpyAsync(nb->doc, T.b_doc, (size_t)T.nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        if (T.nnz) HIP_TRY(h, hipMemcpyAsync(nb->wf, T.b_w, (size_t)T.nnz * sizeof(float), hipMemcpyDeviceToDevice, st));
        return RAG_OK;
    };
    if (int rc = bm_finish_segment(B, nb.get(), enqueue())) return rc;
    h->sparse = nb.release();
    h->sparse_stale = false;
    h->sparse_compacted = false;
    return RAG_OK;
}

// ... and from host arrays of the same layout (rag_sparse_append_docs_host): staged, then the device path
int sparse_append_docs_host(rag_ctx* h, const int32_t* doc_ptr, const int32_t* terms, const float* weights, int64_t n, int64_t nnz_cap,
                            int64_t n_terms_total) {
    const bm_slot S = bm_slot_sparse(h);
    const std::string w = std::string(S.append_name) + ": ";
    ARG_CHECK(h, n >= 1 && n < 0x7fffffff, w + "n_docs_new must be >= 1 (and the index stay under 2^31 documents)");
    ARG_CHECK(h, nnz_cap >= 0 && nnz_cap <= 0x7fffffff, w + "nnz_cap must lie in [0, 2^31)");
    ARG_CHECK(h, doc_ptr && (nnz_cap == 0 || (terms && weights)), w + "null pointer");
    const int64_t used = std::min<int64_t>(std::max<int64_t>(doc_ptr[n], 0), nnz_cap);      // what the kernels may read
    dev_buf<int32_t> ptr_d, terms_d;
    dev_buf<float> w_d;
    int rc;
    if ((rc = bm_alloc(h, ptr_d, (size_t)n + 1, S.append_name))) return rc;
    if ((rc = bm_alloc(h, terms_d, (size_t)used, S.append_name))) return rc;
    if ((rc = bm_alloc(h, w_d, (size_t)used, S.append_name))) return rc;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(ptr_d, doc_ptr, (size_t)(n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (used) HIP_TRY(h, hipMemcpyAsync(terms_d, terms, (size_t)used * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (used) HIP_TRY(h, hipMemcpyAsync(w_d, weights, (size_t)used * sizeof(float), hipMemcpyHostToDevice, st));
    rc = sparse_append_docs_dev(h, ptr_d, terms_d, w_d, n, nnz_cap, n_terms_total);
    (void)hipStreamSynchronize(st);                     // the staged copies read the caller's arrays
    return rc;
}

// rag_sparse_clear
int sparse_clear(rag_ctx* h) {
    sparse_free(h);
    h->sparse_stale = false;
    h->sparse_compacted = false;
    return RAG_OK;
}

// rag_sparse_export_host: base and tail as ONE term-major CSR with global document numbers - each term's base list, then its
// tail list (the order of a fold, and of LexicalPostings.extend). Null arrays: the sizes only.
int sparse_export_host(rag_ctx* h, int64_t* indptr_out, int32_t* doc_out, float* weight_out, int64_t* n_docs_out, int64_t* n_terms_out,
                       int64_t* nnz_out) {
    const rag_bm25_index* ix = h->sparse;
    if (ix == nullptr) {
        h->err = "sparse_export: no sparse postings loaded";
        return RAG_ERR_STATE;
    }
    const rag_bm25_index* tl = ix->tail.get();
    const int64_t V = bm_known_terms(ix), nnz = ix->nnz + (tl ? tl->nnz : 0);
    if (n_docs_out) *n_docs_out = bm_total_docs(ix);
    if (n_terms_out) *n_terms_out = V;
    if (nnz_out) *nnz_out = nnz;
    if (indptr_out == nullptr && doc_out == nullptr && weight_out == nullptr) return RAG_OK;
    ARG_CHECK(h, indptr_out && (nnz == 0 || (doc_out && weight_out)), "sparse_export: null output");
    const std::vector<int64_t> merged = bm_merged_offsets(ix->indptr_h.data(), ix->n_terms, tl ? tl->indptr_h.data() : nullptr, tl ? tl->n_terms : 0, V);
    std::copy(merged.begin(), merged.end(), indptr_out);
    if (tl == nullptr) {
        if (nnz) HIP_TRY(h, hipMemcpyAsync(doc_out, ix->doc, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        if (nnz) HIP_TRY(h, hipMemcpyAsync(weight_out, ix->wf, (size_t)nnz * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return RAG_OK;
    }
    std::vector<int32_t> bd((size_t)ix->nnz), td((size_t)tl->nnz);
    std::vector<float> bw((size_t)ix->nnz), tw((size_t)tl->nnz);
    if (ix->nnz) HIP_TRY(h, hipMemcpyAsync(bd.data(), ix->doc, bd.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (ix->nnz) HIP_TRY(h, hipMemcpyAsync(bw.data(), ix->wf, bw.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (tl->nnz) HIP_TRY(h, hipMemcpyAsync(td.data(), tl->doc, td.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (tl->nnz) HIP_TRY(h, hipMemcpyAsync(tw.data(), tl->wf, tw.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t t = 0; t < V; ++t) {
        int64_t o = merged[(size_t)t];
        if (t < ix->n_terms)
            for (int64_t p = ix->indptr_h[(size_t)t]; p < ix->indptr_h[(size_t)t + 1]; ++p, ++o) { doc_out[o] = bd[(size_t)p]; weight_out[o] = bw[(size_t)p]; }
        if (t < tl->n_terms)
            for (int64_t p = tl->indptr_h[(size_t)t]; p < tl->indptr_h[(size_t)t + 1]; ++p, ++o) {
                doc_out[o] = td[(size_t)p] + (int32_t)tl->row0;
                weight_out[o] = tw[(size_t)p];
            }
    }
    return RAG_OK;
}

// base and tail together
int sparse_info(const rag_ctx* h, int64_t* n_docs_out, int64_t* n_terms_out, int64_t* nnz_out, int64_t* hbm_bytes_out) {
    const rag_bm25_index* ix = h->sparse;
    const rag_bm25_index* tl = ix ? ix->tail.get() : nullptr;
    if (n_docs_out) *n_docs_out = ix ? bm_total_docs(ix) : 0;
    if (n_terms_out) *n_terms_out = ix ? bm_known_terms(ix) : 0;
    if (nnz_out) *nnz_out = ix ? ix->nnz + (tl ? tl->nnz : 0) : 0;
    if (hbm_bytes_out) *hbm_bytes_out = ix ? bm_segment_bytes(ix) + (tl ? bm_segment_bytes(tl) : 0) : 0;
    return RAG_OK;
}

// without a dense index of the same rows the ids are row numbers and there is nothing a tenant could be looked up in
// (per-query tenants: some query is filtered, so the check is a filter's - as in bm25_tenant_args)
static int sparse_args(rag_ctx* h, const void* term_ptr, const void* qweights, int tenant, query_tenants qt = {nullptr, nullptr}) {
    ARG_CHECK(h, h->sparse != nullptr, "no sparse index loaded (rag_sparse_load_host)");
    ARG_CHECK(h, term_ptr != nullptr && qweights != nullptr, "sparse: null query arrays");
    if (int rc = bm25_check_fresh(h, h->sparse)) return rc;
    if (qt.host != nullptr) tenant = 0;
    ARG_CHECK(h, tenant < 0 || (h->index_loaded && h->tenants != nullptr && h->n_rows == bm_total_docs(h->sparse)),
              "sparse: a tenant filter needs a dense index of the same rows with rag_index_set_tenants_host");
    return RAG_OK;
}

int sparse_topk_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, const float* qweights, int Q, int k, int tenant,
                     int64_t* ids_out, int32_t* rows_out, double* scores_out, query_tenants qt) {
    ARG_CHECK(h, ids_out && scores_out, "sparse_topk: null output");
    if (int rc = sparse_args(h, term_ptr, qweights, tenant, qt)) return rc;
    return bm25_run(h, h->sparse, term_ptr, terms, Q, k, 0, tenant, ids_out, rows_out, scores_out, nullptr, nullptr, qt, qweights);
}

int sparse_scores_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, const float* qweights, int Q, double* out) {
    ARG_CHECK(h, out, "sparse_scores: null output");
    if (int rc = sparse_args(h, term_ptr, qweights, -1)) return rc;
    return bm25_run(h, h->sparse, term_ptr, terms, Q, 1, 1, -1, nullptr, nullptr, nullptr, nullptr, out, {nullptr, nullptr}, qweights);
}

int sparse_topk_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev, int Q, int k, int tenant,
                    int64_t* ids_dev, int32_t* rows_dev, double* scores_dev, hipStream_t st, id_space ids, query_tenants qt) {
    if (int rc = sparse_args(h, term_ptr_dev, qweights_dev, tenant, qt)) return rc;
    return bm_topk_dev(h, h->sparse, term_ptr_dev, terms_dev, qweights_dev, Q, k, tenant, ids_dev, rows_dev, scores_dev, nullptr, st, ids, qt);
}

// ---- point lookup: the exact learned-sparse score of GIVEN rows (rag_sparse_score_rows_*; the sparse component of rag_m3_score_rows_dev)
// The range kernel scores whole 2048-document ranges and the top-k reports a document only if it made the list; a weighted sum
// over candidates another leg found needs s(q, row) for an arbitrary row. One 256-thread workgroup per query. The query's tokens
// are staged in LDS in chunks of at most 256: the term's bm_term_meta in the base and in the tail (df = 0: the segment does not
// know the term, or the token adds nothing) and the float32 weight widened to float64. Wave w takes the slots w, w + 4, ...;
// inside a wave lane = token: bm_bracket at the row, bm_search, one compare of the found doc id, one weight load - every lookup
// of a slot is independent of the others. Only the sum is ordered: a lane that finds nothing holds +0.0, and the wave adds the
// lanes' products in lane order = token order into the slot's accumulator (kept in a register of lane `slot / 4` across the 64-token
// groups and the LDS chunks). Adding +0.0 to a non-negative float64 changes nothing, so the sum is the range kernel's - which adds
// exactly the postings that exist, in token order - bit for bit. A row lives in one segment (base: row < n_docs, tail: local
// document row - row0), as its accumulator does in the searches. No atomics, no LDS accumulators, no plan table.
struct bm_point_seg { const bm_term_meta* meta; const int32_t* doc; const float* wf; const int32_t* range_tab; int64_t n_terms; };
#define BM_POINT_CHUNK 256

__device__ __forceinline__ double bm_readlane_f64(double v, int i) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, i), hi = (uint32_t)__builtin_amdgcn_readlane((int)(u >> 32), i);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(256) void sparse_point_kernel(const bm_point_seg sb, const bm_point_seg stl, int64_t base_docs, int64_t total_docs,
                                                            int64_t tail_row0, const int32_t* __restrict__ term_ptr,
                                                            const int32_t* __restrict__ terms, const float* __restrict__ qweights,
                                                            const int32_t* __restrict__ cand, int pool, double* __restrict__ out) {
    __shared__ bm_term_meta s_meta[2][BM_POINT_CHUNK];
    __shared__ double s_qw[BM_POINT_CHUNK];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = term_ptr[q], t1 = term_ptr[q + 1];
    double acc = 0.0;                                          // lane l: the accumulator of slot wv + 4 l
    for (int tb = t0; tb < t1; tb += BM_POINT_CHUNK) {
        const int nb = min(BM_POINT_CHUNK, t1 - tb);
        if (tb != t0) __syncthreads();                         // the previous chunk has been read by every wave
        if (tid < nb) {
            const int t = terms[tb + tid];
            const float qw = qweights[tb + tid];
            const bool live = qw > 0.0f;                       // a weight that is not > 0 (NaN included) adds nothing
            const bm_term_meta none = {0, 0, 0.0, 0, BM_NO_TAB};
            s_meta[0][tid] = live && t >= 0 && t < sb.n_terms ? sb.meta[t] : none;
            s_meta[1][tid] = live && t >= 0 && t < stl.n_terms ? stl.meta[t] : none;
            s_qw[tid] = live ? (double)qw : 0.0;
        }
        __syncthreads();
        for (int s = 0; wv + 4 * s < pool; ++s) {
            const int row = cand[(size_t)q * pool + wv + 4 * s];                                 // (wave-uniform)
            if (row < 0 || row >= total_docs) continue;
            const int seg = row >= base_docs ? 1 : 0;
            const bm_point_seg& S = seg ? stl : sb;
            const int64_t local = seg ? row - tail_row0 : (int64_t)row;
            double a = __shfl(acc, s);
            for (int c = 0; c < nb; c += 64) {
                double prod = 0.0;
                if (c + lane < nb) {
                    const bm_term_meta m = s_meta[seg][c + lane];
                    if (m.df > 0) {
                        int lo, hi;
                        bm_bracket(m, S.range_tab, local, lo, hi);
                        const int p = bm_search(S.doc + m.post, lo, hi, local);
                        if (p < m.df && S.doc[m.post + p] == local) prod = s_qw[c + lane] * (double)S.wf[m.post + p];
                    }
                }
                uint64_t found = __ballot(prod != 0.0);
                while (found) {                                // in lane order = token order
                    const int i = __builtin_ctzll(found);
                    a += bm_readlane_f64(prod, i);
                    found &= found - 1;
                }
            }
            if (lane == s) acc = a;
        }
    }
    const int j = wv + 4 * lane;
    if (j < pool) out[(size_t)q * pool + j] = acc;
}

static int sparse_point_usable(rag_ctx* h) {
    if (!h->sparse) {
        h->err = "sparse_score_rows: no sparse index loaded (rag_sparse_load_host)";
        return RAG_ERR_STATE;
    }
    return bm25_check_fresh(h, h->sparse);
}

// scores_dev [Q][pool] float64 <- s(query q, row cand_rows_dev[q][j]); everything on the device, asynchronous on st
int sparse_score_rows_dev(rag_ctx* h, const int32_t* term_ptr_dev, const int32_t* terms_dev, const float* qweights_dev,
                          const int32_t* cand_rows_dev, int Q, int pool, double* scores_dev, hipStream_t st) {
    if (int rc = sparse_point_usable(h)) return rc;
    ARG_CHECK(h, Q > 0 && Q <= 65535 && pool > 0 && pool <= RAG_MAX_K, "sparse_score_rows: 1 <= n_queries <= 65535, 0 < pool <= 256");
    ARG_CHECK(h, term_ptr_dev && qweights_dev && cand_rows_dev && scores_dev, "sparse_score_rows: null argument");
    const rag_bm25_index* ix = h->sparse;
    const rag_bm25_index* tl = ix->tail.get();
    const bm_point_seg sb = {ix->meta, ix->doc, ix->wf, ix->range_tab, ix->n_terms};
    const bm_point_seg stl = tl ? bm_point_seg{tl->meta, tl->doc, tl->wf, tl->range_tab, tl->n_terms} : bm_point_seg{nullptr, nullptr, nullptr, nullptr, 0};
    launch(sparse_point_kernel, dim3((unsigned)Q), dim3(256), 0, st, sb, stl, ix->n_docs, tl ? bm_total_docs(ix) : ix->n_docs, tl ? tl->row0 : (int64_t)0,
           term_ptr_dev, terms_dev, qweights_dev, cand_rows_dev, pool, scores_dev);
    return launch_status(h);
}

int sparse_score_rows_host(rag_ctx* h, const int32_t* term_ptr, const int32_t* terms, const float* qweights, const int32_t* cand_rows, int Q,
                           int pool, double* scores_out) {
    if (int rc = sparse_point_usable(h)) return rc;
    ARG_CHECK(h, Q > 0 && Q <= 65535 && pool > 0 && pool <= RAG_MAX_K, "sparse_score_rows: 1 <= n_queries <= 65535, 0 < pool <= 256");
    ARG_CHECK(h, term_ptr && cand_rows && scores_out, "sparse_score_rows: null argument");
    ARG_CHECK(h, term_ptr[0] >= 0, "sparse_score_rows: term_ptr must start at >= 0 and never decrease");
    for (int q = 0; q < Q; ++q) ARG_CHECK(h, term_ptr[q + 1] >= term_ptr[q], "sparse_score_rows: term_ptr must start at >= 0 and never decrease");
    const size_t nt = (size_t)term_ptr[Q], P = (size_t)Q * pool;
    ARG_CHECK(h, nt == 0 || (terms && qweights), "sparse_score_rows: null query arrays");
    hipStream_t st = h->stream;
    dev_buf<int32_t> dtp, dtm, dcand;
    dev_buf<float> dqw;
    dev_buf<double> dsc;
    int rc;
    if ((rc = dtp.alloc(h, (size_t)Q + 1)) || (rc = dtm.alloc(h, std::max<size_t>(nt, 1))) || (rc = dqw.alloc(h, std::max<size_t>(nt, 1))) ||
        (rc = dcand.alloc(h, P)) || (rc = dsc.alloc(h, P)))
        return rc;
    HIP_TRY(h, hipMemcpyAsync(dtp, term_ptr, ((size_t)Q + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (nt) HIP_TRY(h, hipMemcpyAsync(dtm, terms, nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (nt) HIP_TRY(h, hipMemcpyAsync(dqw, qweights, nt * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(dcand, cand_rows, P * sizeof(int32_t), hipMemcpyHostToDevice, st));
    rc = sparse_score_rows_dev(h, dtp, dtm, dqw, dcand, Q, pool, dsc, st);
    if (!rc) HIP_TRY(h, hipMemcpyAsync(scores_out, dsc, P * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return rc;
}
