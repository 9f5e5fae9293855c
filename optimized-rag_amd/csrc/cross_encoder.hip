// K7: BertForSequenceClassification forward (ms-marco-MiniLM-L-6-v2 shape: 6 layers, hidden 384, 12 heads x 32,
// FFN 1536, 1 logit). Replaces `self.model.predict(pairs)` of CrossEncoderReranker.rerank
// (/root/reference/rag/reranker.py:355); sigmoid and sorting stay in the Python mirror (:359,:373).
//
// Numerics: the north star asks for rerank scores within 1e-3. Single fp16 operands give ~2e-2 logit error after
// 6 layers (measured), so every MFMA operand is a SPLIT fp16 pair x = hi + lo (hi = fp16(x), lo = fp16(x - hi),
// ~22 significand bits) stored as two planes, and every product is 3 MFMAs: hi*hi + hi*lo + lo*hi with fp32
// accumulation (3/16 of the f32-MFMA cost for the same accuracy class). GEMM operands (weights, x, ctx, q, ffn activations)
// keep the two halves INTERLEAVED per 32-element K group: [hi 32 halfs | lo 32 halfs] = 128 B, so the row piece one K-step
// (32 elements) stages is one whole 128-B line instead of two 64-B halves of two lines (SPLIT_IDX). Residual stream / LayerNorm / softmax /
// GELU (erf form, A&S 7.1.26) / pooler are fp32. Layout: tokens are rows, PACKED per pair (offsets computed on the device),
// feature contiguous; weights are nn.Linear [out][in] = K-contiguous, so every GEMM is the "both operands K-contiguous" form
// MFMA wants. The packing has TWO row spaces. Attention space: pair p owns len_p rounded up to 16 rows (pair_off) - the Q / K / V
// fragment tiles are 16 rows of one pair. GEMM row space: pair p owns len_p rounded up to g rows (row_off) - embeddings, every
// GEMM operand and result, LayerNorm, GELU and the attention context. g = 4 in the MX forward of a classifier (the GEMMs' 128-row
// tiles do not care where a pair starts; 4 is what the V epilogue's four-key store needs), which so computes 1.5 pad rows per pair
// on average instead of 7.5; g = 16 - one row space, row_off = pair_off - in the split-fp16 forward and for embedding models, whose
// pooling and token heads read rows through pair_off. The QKV epilogue maps a GEMM row to its attention row (row_att), attention
// writes its context back to GEMM rows, and the slots of a pair's last attention tile past its GEMM rows are written by nobody:
// K there is masked after the MFMA, V there is zeroed (LDS) or selected to zero (DIRECT) by the attention kernel.
//
// Kernels
//   ce_pack_scan/rows  lens -> pair_off / row_off / row_pair / row_att / m_packed (the packed row layout of the chunk)
//   ce_embed_ln        word+pos+type gather -> LayerNorm -> x16: the residual stream IS the split-fp16 GEMM operand (hi + lo
//                      = 22 significant bits); there is no separate fp32 copy
//   ce_gemm<EPI>       persistent, XCD-aware; 128 (out features) x 256 (tokens) tiles, BK = 32, three LDS stages by
//                      LDS-DMA with a continuous stream across tiles, 8 staggered waves (2 x 4 of 64 x 64), source-swizzled
//                      conflict-free ds_read_b128. Output features sit on the MFMA ROW (bias = 4 registers per lane).
//                      Epilogues through the free ring stage, non-temporal stores: QKV (Q token-major; K and V in MFMA
//                      FRAGMENT order per (pair, head)), bias + GELU -> split fp16, bias + residual -> fp32.
//   ce_attention<QB>   one workgroup per (head, pair); K/V fragments by LDS-DMA, S computed transposed so that P stays in
//                      registers as the next MFMA's operand, online softmax over 32-key blocks, keys past len skipped.
//   ce_attention64     the same scheme for models with 64-wide heads (BERT-base / BERT-large shapes; EPI_QKV64 writes their K / V
//                      tiles): S chains two MFMAs over the head's dim halves, P.V fills four 16-dim accumulators; LDS-staged
//                      up to length class 256, fragments read from global memory at 384 and 512, streamed through an LDS ring
//                      shared by a workgroup's waves in the classes 768 ... 8192
//   ce_layernorm       one wave per token (384 = 6/lane), fp32 statistics, eps from config
//   ce_pool_classify   tanh(Wp.x_cls + bp) -> wc.pooled + bc, fp32
//   ce_meanpool        embedding head: mean over the real tokens, or the [CLS] row; optional L2 normalisation
//   m3_*               the embedder's optional token-vector and lexical heads (rag_embed_multi_*): ce_gemm<EPI_F32> over the last
//                      hidden state, then normalise + scatter to packed rows; one dot per row for the lexical weights
// One layer, in launch order: QKV GEMM, attention, out-projection GEMM (bias + residual -> fp32) + LayerNorm, FFN-up GEMM
// (bias + GELU) + FFN-down GEMM (bias + residual -> fp32) + LayerNorm. These split-fp16 kernels run every model whose shape
// the MX forward (ce_mx.h: hi16 + lo8 operands, hidden 384) does not take, classifiers whose load-time probe saw MX miss
// (ce_probe_mx), and option ce_mx = -1.
#include "common.h"
#include "ce_mx.h"
#include <type_traits>

#include <cmath>
#include <cstdlib>
#include <cstring>

// one chunk's token arrays, packed row layout and host staging (sized for `pairs` pairs of L tokens, Mp padded rows). Each
// forward has an instance of its own, so switching between them (option ce_mx) never resizes the other forward's buffers.
struct ce_chunk_bufs {
    dev_buf<int32_t> ids, tt, lens;                                    // [Mp] token / type ids padded to L, [pairs] lengths
    dev_buf<int32_t> clen;                                             // [pairs] lengths clamped to [1, L_in]: what every kernel after the scan reads
    // packed (variable-length) row layout of the current chunk, in two row spaces. ATTENTION space: pair p owns rows
    // [pair_off[p], pair_off[p+1]), its length rounded up to 16 (whole Q / K / V fragment tiles). GEMM row space (activations, the
    // residual stream): pair p owns rows [row_off[p], row_off[p+1]), its length rounded up to the forward's granularity g: 4 in the MX
    // forward of a classifier, else 16, where the two spaces coincide. row_pair[m] = owning pair of GEMM row m (-1 past the end),
    // row_att[m] = its attention row (-1 past the end); m_packed[0] = row_off[P] = GEMM rows
    dev_buf<int32_t> pair_off, row_off, row_pair, row_att, m_packed;
    dev_buf<int32_t> sid, stt;                                         // staging of one chunk's [pairs][L_in] token / type ids
    dev_buf<float> logits;                                             // staging of one chunk's outputs, [pairs][out_width]
};

// What the activation workspaces of both forwards share. Each forward adds its own planes (ce_ensure_ws / mx_ensure_ws);
// a workspace is dropped by assigning an empty one.
struct ce_ws_base {
    int pairs = 0, L = 0;                              // what the workspace was allocated for (0: nothing fits)
    int64_t tokens = 0;                                // padded rows (a multiple of 256): every plane stride follows it
    ce_chunk_bufs io;
    bool fits(int P, int L_) const { return P <= pairs && L_ == L; }
};
struct ce_split_ws : ce_ws_base {
    dev_buf<float> y32;                                // pre-LayerNorm sums of the residual GEMMs (fp32 [tokens][hidden])
    dev_buf<half_t> x16, q16, kf16, vf16, ctx16, h16;
};
struct ce_mx_ws : ce_ws_base {
    dev_buf<char> x8, ctx8, h8;                        // residual stream, attention output, FFN intermediate (image layout)
    dev_buf<char> xc8, cc8, hc8;                       // the same three for ONE row per pair: the [CLS] rows through the last layer's tail
    dev_buf<char> ffn_slots;                           // fused FFN (mx_ffn_kernel): one token tile of the intermediate per workgroup; h8 / hc8 are then not allocated (mx_ensure_ffn)
    dev_buf<int32_t> m_cls;                            // device scalar: rows of the compact tensors (= pairs of the chunk)
    dev_buf<half_t> qf16, kf16, vf16;                  // Q, K, V in the attention kernel's fragment order (hi | lo planes)
};

// The optional heads of an embedder (rag_embed_heads_load_host) and what one rag_embed_multi_* call asks of them.
struct ce_heads {
    int tok_dim = 0, tok_pad = 0;                      // token head: output width, and that width rounded up to the GEMM's 128-feature tile
    dev_buf<half_t> tok_w;                             // [tok_pad][hidden] split fp16, rows past tok_dim zero
    dev_buf<float> tok_b;                              // [tok_pad], zero where the checkpoint has no bias
    dev_buf<float> lex_w;                              // [hidden] fp32 (empty: no lexical head)
    float lex_b = 0.f;
    // scratch of a multi call, sized with the forward's workspace: the MX forward's last hidden state in the split layout, and
    // the token head's rows before normalisation (fp32 [tokens][tok_pad])
    dev_buf<half_t> x16;
    dev_buf<float> raw;
    int64_t x16_tokens = 0, raw_tokens = 0;
};
// lex / tok: the call's outputs (device, or null); row_off [P + 1] = the packed row each text's token vectors start at
struct ce_multi {
    float* lex;
    float* tok;
    int64_t* row_off;                                  // written by the call itself (m3_row_off_kernel) before its first chunk
    int64_t tok_cap;
};

struct rag_ce_model {
    rag_ce_config cfg;
    ce_heads heads;
    bool embed = false;          // true: sentence-embedding encoder (mean or [CLS] pooling over the tokens, no pooler / classifier head)
    int normalize = 1;           // embed: L2-normalise the pooled vectors
    int pool_cls = 0;            // embed: pool by the [CLS] row (the last hidden state of row 0) instead of the mean
    int d_head = 32;             // 32, or 64: the split-fp16 forward with the EPI_QKV64 epilogue and ce_attention64_kernel
    int out_width = 1;           // floats per pair the forward produces: 1 logit, or `hidden` for an embedding model
    // embeddings fp32
    dev_buf<float> word, pos, type, emb_ln_g, emb_ln_b;
    struct Layer {
        dev_buf<half_t> wqkv, wo, w1, w2;              // fp16 [out][in]
        dev_buf<char> wqkv8, wo8, w18, w28;            // the same matrices as hi16 + lo8 images (ce_mx.h), when the shape allows
        dev_buf<float> bqkv, bo, b1, b2;
        dev_buf<float> ln1_g, ln1_b, ln2_g, ln2_b;
    };
    std::vector<Layer> layers;
    dev_buf<float> wp, bp, wc, bc;                     // pooler / classifier fp32
    dev_buf<float> wpT;                                // pooler matrix transposed (mx_pool_classify_kernel)
    // the MX forward (ce_mx.h: hi16 + lo8 operands) runs every model whose shape allows it, the split-fp16 kernels the others
    // (and option ce_mx = -1); each has a workspace of its own, and neither path must size or evict the other's buffers
    bool mx_ok = false;                                // the shape allows the MX path (hidden 384, ffn a multiple of 384 up to 1536) and its weights are loaded
    bool mx_default = true;                            // option ce_mx = 0 takes the MX path: false when the load-time probe (ce_probe_mx) saw it miss
    ce_split_ws split;
    ce_mx_ws mx;
};

#define CE_BM 128     // output features per tile (MFMA rows)
#define CE_BN 256     // tokens per tile (MFMA cols)
#define CE_BK 32      // K per LDS stage = one mfma_16x16x32 k-step
#define CE_W_TILE (CE_BM * 128)                           // weight tile of one K-step: 128 rows x [hi 64 B | lo 64 B] = 16 KiB
#define CE_X_TILE (CE_BN * 128)                           // token tile of one K-step: 256 rows x 128 B = 32 KiB
#define CE_STAGE_BYTES (CE_W_TILE + CE_X_TILE)            // 48 KiB
// element c of a split row lives at half index SPLIT_IDX(c) (hi) and SPLIT_IDX(c) + 32 (lo); a row of n elements takes 2n halfs
#define SPLIT_IDX(c) ((((c) >> 5) << 6) + ((c) & 31))
#define CE_GEMM_LDS (3 * CE_STAGE_BYTES)                  // three stages = 144 KiB
#define CE_EPI_PLANE16 (16 * 144)                         // one fp16 plane of a 16-token x 64-feature epilogue pass, rows padded to 144 B

// EPI_QKV64: the QKV epilogue of a model with 64-wide heads (K and V fragment tiles of ce_attention64_kernel)
// EPI_F32: bias -> fp32 [token][N] with no residual (the token-vector head of the embedder, before its normalisation)
enum { EPI_QKV = 0, EPI_GELU = 1, EPI_RESID = 2, EPI_QKV64 = 3, EPI_F32 = 4 };

__device__ __forceinline__ void store_split4(half_t* __restrict__ p, size_t plane, float v0, float v1, float v2, float v3) {
    const half4 hi = {(half_t)v0, (half_t)v1, (half_t)v2, (half_t)v3};
    const half4 lo = {(half_t)(v0 - (float)hi[0]), (half_t)(v1 - (float)hi[1]), (half_t)(v2 - (float)hi[2]),
                      (half_t)(v3 - (float)hi[3])};
    *reinterpret_cast<half4*>(p) = hi;
    *reinterpret_cast<half4*>(p + plane) = lo;
}

// LDS rows are 128 B (8 chunks of 16 B: hi chunks 0-3, lo chunks 4-7 of one 32-element K group). Chunk c of row r is
// stored at position c ^ ((r>>1) & 7) - dense.hip's swizzle, conflict-free for ds_read_b128 fragment reads - applied on the
// DMA SOURCE address; the LDS destination stays lane-linear.
// LDS-DMA piece through a buffer descriptor: per-lane byte offset in ONE VGPR, piece / K-step offset in a scalar register
// (no 64-bit address arithmetic per piece; reads past the descriptor's end return zeros)
__device__ __forceinline__ void ce_bdma(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, char* lds, int wid) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + wid * 64 * 16), 16, voff, soff, 0, 0);
}

// C^T[n][m] = sum_k W[n][k] * X[m][k].   W: [2 planes][N][K] fp16, X: [2 planes][M_pad][K] fp16 (hi plane, then lo).
// N % 128 == 0, M_pad % 256 == 0, K % 32 == 0, K >= 64.
// 128 (features) x 256 (tokens) tile, 8 waves (2 x 4, each 64 x 64), BK = 32, THREE LDS stages filled by LDS-DMA two
// K-steps ahead. Same staggered structure as dense.hip: per K-step an I-part (16 fragment reads + 6 DMA pieces,
// lgkmcnt(0)) and an M-part (48 MFMAs = 16 products x {lo*hi, hi*lo, hi*hi}), each closed by s_barrier; waves 4-7 run
// half a phase behind waves 0-3 so one group's MFMAs cover the other's reads. RAW: one counted s_waitcnt vmcnt(6)
// per K-step (step t+1 landed, step t+2 in flight); WAR: stage (t+2)%3 was last read in I(t-1).
//
// PERSISTENT workgroups (one per CU) with a CONTINUOUS DMA stream across tiles: the K = 384 GEMMs have only 12 K-steps, so
// a per-tile prologue (two stages from cold) and epilogue cost a quarter of the tile. The last two K-steps of a tile
// therefore issue steps 0 and 1 of the workgroup's NEXT tile into the stage ring, and the epilogue transposes through
// the one stage that is free at that point (48 KiB = 6 KiB per wave, four 16-token passes), so the next main loop
// starts with both stages resident. The packed row count lives on the device (no host sync): the loop stops at the
// first token tile past it.
#define CE_EPI_WAVE_BYTES (CE_STAGE_BYTES / 8)            // 6 KiB of the free stage per wave
template <int EPI>
__global__ __launch_bounds__(512) void ce_gemm_kernel(const half_t* __restrict__ W, const half_t* __restrict__ X,
                                                       int N, int K, const float* __restrict__ bias,
                                                       const half_t* __restrict__ resid, float* __restrict__ out32,
                                                       half_t* __restrict__ out16, half_t* __restrict__ kf16,
                                                       half_t* __restrict__ vf16, size_t kv_plane, int hidden, int heads,
                                                       const int32_t* __restrict__ m_packed, int m_pad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 2, wn = wid & 3;
    const bool lag = wm != 0;
    const int n_ft = N / CE_BM;
    const int m_end = m_packed[0];
    // XCD-aware work order (speed only): workgroup b runs on XCD b & 7, and every XCD has its own L2. XCD x owns the token
    // tiles m = x (mod 8); its gridDim.x / 8 workgroups walk the (token tile, feature tile) pairs of those tiles feature
    // tile fastest, so the n_ft workgroups that share a token tile read it through ONE L2 (before this, the tile was
    // fetched once per XCD: 20 GB of HBM/fabric reads per FFN-up GEMM against 2.3 GB of activations).
    const int xcd = blockIdx.x & 7, n_slots = gridDim.x >> 3;
    int work = blockIdx.x >> 3;
#define CE_TILE_M(w) (((w) / n_ft) * 8 + xcd)
#define CE_TILE_N(w) ((w) % n_ft)
    if (CE_TILE_M(work) * CE_BN >= m_end) return;
    // DMA source per thread: one piece = 64 rows x 128 B; linear chunk i = tid: row i>>3, position i&7 -> source chunk
    // (i&7) ^ ((row>>1)&7); (row + 64)>>1 has the same low 3 bits, so every piece of a tile uses the same per-thread chunk
    const int sr = tid >> 3;                                          // 0..63
    const int schunk = (tid & 7) ^ ((sr >> 1) & 7);
    const size_t ldk = (size_t)2 * K;                                 // halfs per split row
    const size_t piece = (size_t)64 * ldk;                            // 64 rows further
    const int fr = lane & 15, fq = lane >> 4;
    // fragment row r = base16 + fr (base16 multiple of 16 -> (r>>1)&7 == (fr>>1)&7): byte offsets of the hi / lo chunk
    const int sw = (fr >> 1) & 7;
    const int off = fr * 128 + ((fq ^ sw) << 4), off_lo = fr * 128 + (((4 + fq) ^ sw) << 4);
    const int a_base = wm * 64 * 128, b_base = CE_W_TILE + wn * 64 * 128;
    const int nt = K / CE_BK;
    const int last = nt - 1;
    // Buffer addressing: W through one descriptor + a scalar tile offset, the 256 token rows of a tile
    // through a per-tile descriptor, ONE per-lane byte offset for all six pieces of a stage. The pointer form spent ~14 VALU
    // instructions per K-step on 64-bit source addresses inside the part of the step that is on the critical path.
    const unsigned voff = (unsigned)(((size_t)sr * ldk + schunk * 8) * sizeof(half_t));
    const unsigned piece_b = (unsigned)(piece * sizeof(half_t));
    const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(W), 0, (int)((size_t)N * ldk * sizeof(half_t)), 0x00020000);
    unsigned w_cur = (unsigned)((size_t)CE_TILE_N(work) * CE_BM * ldk * sizeof(half_t)), w_nxt = w_cur;      // byte offset of the feature tile
    __amdgpu_buffer_rsrc_t x_cur = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(X + (size_t)CE_TILE_M(work) * CE_BN * ldk), 0,
                                                                     (int)(4 * piece_b), 0x00020000);
    __amdgpu_buffer_rsrc_t x_nxt = x_cur;
    bool has_next = false;
    int sbase = 0;                               // ring stage of step 0 of the current tile
#define CE_ISSUE(u)   /* step u of the current tile; u >= nt: step u - nt of the next tile (or a harmless re-load) */     \
    {                                                                                                             \
        const int u_ = (u);                                                                                       \
        const bool nx_ = u_ >= nt && has_next;                                                                    \
        const unsigned ks_ = (unsigned)(u_ < nt ? u_ : (has_next ? u_ - nt : last)) * 128u;                       \
        const unsigned ws_ = (nx_ ? w_nxt : w_cur) + ks_;                                                         \
        char* st_ = smem + ((sbase + u_) % 3) * CE_STAGE_BYTES;                                                   \
        ce_bdma(w_rs, voff, ws_, st_, wid);                                                                       \
        ce_bdma(w_rs, voff, ws_ + piece_b, st_ + 8192, wid);                                                      \
        if (nx_) {                                                                                                \
            ce_bdma(x_nxt, voff, ks_, st_ + CE_W_TILE, wid);                                                      \
            ce_bdma(x_nxt, voff, ks_ + piece_b, st_ + CE_W_TILE + 8192, wid);                                     \
            ce_bdma(x_nxt, voff, ks_ + 2 * piece_b, st_ + CE_W_TILE + 2 * 8192, wid);                             \
            ce_bdma(x_nxt, voff, ks_ + 3 * piece_b, st_ + CE_W_TILE + 3 * 8192, wid);                             \
        } else {                                                                                                  \
            ce_bdma(x_cur, voff, ks_, st_ + CE_W_TILE, wid);                                                      \
            ce_bdma(x_cur, voff, ks_ + piece_b, st_ + CE_W_TILE + 8192, wid);                                     \
            ce_bdma(x_cur, voff, ks_ + 2 * piece_b, st_ + CE_W_TILE + 2 * 8192, wid);                             \
            ce_bdma(x_cur, voff, ks_ + 3 * piece_b, st_ + CE_W_TILE + 3 * 8192, wid);                             \
        }                                                                                                         \
    }
#define CE_BAR __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0);
    CE_ISSUE(0)
    CE_ISSUE(1)
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    CE_BAR
    for (bool first = true;; first = false) {
        const int n0 = CE_TILE_N(work) * CE_BM;  // feature tile
        const int m0 = CE_TILE_M(work) * CE_BN;  // token tile
        const int nb = n0 + wm * 64, mb = m0 + wn * 64;
        {
            const int nx = work + n_slots;
            has_next = CE_TILE_M(nx) * CE_BN < m_end;
            if (has_next) {
                w_nxt = (unsigned)((size_t)CE_TILE_N(nx) * CE_BM * ldk * sizeof(half_t));
                x_nxt = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(X + (size_t)CE_TILE_M(nx) * CE_BN * ldk), 0, (int)(4 * piece_b), 0x00020000);
            }
        }
        // bias in registers before the main loop: the epilogue must not start with a global load behind the in-flight DMA
        float4 bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[i] = *reinterpret_cast<const float4*>(bias + nb + i * 16 + fq * 4);
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (lag) { CE_BAR }
        for (int t = 0; t < nt; ++t) {
            const char* st = smem + ((sbase + t) % 3) * CE_STAGE_BYTES;
            half8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ah[i] = *reinterpret_cast<const half8*>(st + a_base + i * 16 * 128 + off);
                al[i] = *reinterpret_cast<const half8*>(st + a_base + i * 16 * 128 + off_lo);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bh[j] = *reinterpret_cast<const half8*>(st + b_base + j * 16 * 128 + off);
                bl[j] = *reinterpret_cast<const half8*>(st + b_base + j * 16 * 128 + off_lo);
            }
            CE_ISSUE(t + 2)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // step t+1 must have landed before the next I-part. On a continued tile steps 0 and 1 were resident before the
            // loop started (see below), so its first wait is skipped: it would only wait for the previous epilogue's stores.
            const bool need_wait = first || t > 0;
            if (lag && need_wait) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            CE_BAR
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // both correction products at every site: dropping either spends the whole logit-error budget
                    // (profiles/r02_b_ce_term_ablation.md)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);       // W_lo * x_hi
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);       // W_hi * x_lo
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
            __builtin_amdgcn_s_setprio(0);
            if (!lag && need_wait) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            CE_BAR
        }
        if (!lag) { CE_BAR }
        // Both groups are past their last fragment reads. Steps 0 and 1 of the next tile are in flight into the other two
        // stages; wait for them here, where no store is outstanding yet (a counted wait across the epilogue's stores
        // would rely on loads and stores retiring in one order).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // epilogue: acc[i][j][r] = C^T[n = nb + i*16 + fq*4 + r][m = mb + j*16 + fr]. Each wave transposes its 64 x 64 tile,
        // 16 tokens (32 for V) at a time, through its 6 KiB of the free stage so that every global store / residual load
        // covers whole 128 B lines of the row-major outputs (or one whole 1 KiB MFMA fragment tile for K and V).
        // outputs are streamed with non-temporal stores: they are read again only by a later kernel (GBs later), and as
        // ordinary stores they pushed the shared token tile and the weights out of the XCD's 4 MiB L2
        char* wl = smem + ((sbase + nt + 2) % 3) * CE_STAGE_BYTES + wid * CE_EPI_WAVE_BYTES;
        if (EPI == EPI_RESID || EPI == EPI_F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {                       // fp32 [16 tokens][64 features], row stride 272 B
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *reinterpret_cast<float4*>(wl + fr * 272 + (i * 16 + fq * 4) * 4) =
                        make_float4(acc[i][j][0] + bv[i].x, acc[i][j][1] + bv[i].y, acc[i][j][2] + bv[i].z, acc[i][j][3] + bv[i].w);
                __builtin_amdgcn_wave_barrier();
                const int rr = lane >> 4, cc = lane & 15;
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int row = it * 4 + rr;
                    const float4 v = *reinterpret_cast<const float4*>(wl + row * 272 + cc * 16);
                    const size_t g = (size_t)(mb + j * 16 + row) * N + nb + cc * 4;
                    if (EPI == EPI_F32) {
                        __builtin_nontemporal_store((f32x4){v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(out32 + g));
                        continue;
                    }
                    const half_t* rp = resid + (size_t)(mb + j * 16 + row) * 2 * N + SPLIT_IDX(nb + cc * 4);      // residual = hi + lo
                    const half4 rh = *reinterpret_cast<const half4*>(rp), rl = *reinterpret_cast<const half4*>(rp + 32);
                    __builtin_nontemporal_store((f32x4){v.x + ((float)rh[0] + (float)rl[0]), v.y + ((float)rh[1] + (float)rl[1]),
                                                        v.z + ((float)rh[2] + (float)rl[2]), v.w + ((float)rh[3] + (float)rl[3])},
                                                reinterpret_cast<f32x4*>(out32 + g));
                }
                __builtin_amdgcn_wave_barrier();
            }
        } else if (EPI == EPI_GELU || nb < 2 * hidden) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {                       // split fp16 [16 tokens][64 features]: hi plane | lo plane, rows 144 B
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v0 = acc[i][j][0] + bv[i].x, v1 = acc[i][j][1] + bv[i].y, v2 = acc[i][j][2] + bv[i].z, v3 = acc[i][j][3] + bv[i].w;
                    if (EPI == EPI_GELU) { v0 = ce_gelu(v0); v1 = ce_gelu(v1); v2 = ce_gelu(v2); v3 = ce_gelu(v3); }
                    store_split4(reinterpret_cast<half_t*>(wl + fr * 144 + (i * 16 + fq * 4) * 2), CE_EPI_PLANE16 / 2, v0, v1, v2, v3);
                }
                __builtin_amdgcn_wave_barrier();
                if (EPI == EPI_GELU || nb < hidden) {
                    // FFN activations [token][ffn], or Q rows [token][hidden], in the split-row layout: the wave's 64 features
                    // of a token are two K groups = [hi 32 | lo 32 | hi 32 | lo 32] = 256 contiguous bytes; 16 lanes cover them
                    const int ldo = 2 * (EPI == EPI_GELU ? N : hidden);
                    const int rr = lane >> 4, cc = lane & 15;
                    const int grp = cc >> 3, part = (cc >> 2) & 1, qtr = cc & 3;
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int row = it * 4 + rr;
                        const half8 v = *reinterpret_cast<const half8*>(wl + part * CE_EPI_PLANE16 + row * 144 + (grp * 4 + qtr) * 16);
                        half_t* o = out16 + (size_t)(mb + j * 16 + row) * ldo + (nb >> 5) * 64 + cc * 8;
                        __builtin_nontemporal_store(v, reinterpret_cast<half8*>(o));
                    }
                } else if (EPI == EPI_QKV64) {
                    // 64-wide heads: the wave's 64 features are ONE head, two 32-dim halves. K features ->
                    // kf16[head][16-row tile][dim half][lane = fq*16 + key%16][8 dims half*32 + fq*8..]: the two A fragments the S chain
                    // of ce_attention64_kernel reads, 2 KiB per (head, tile) and plane. One store = one whole 1 KiB fragment tile.
                    const int head = (nb - hidden) >> 6;
                    const int m = mb + j * 16;
#pragma unroll
                    for (int dh = 0; dh < 2; ++dh) {
                        const half8 hi = *reinterpret_cast<const half8*>(wl + fr * 144 + (dh * 4 + fq) * 16);
                        const half8 lo = *reinterpret_cast<const half8*>(wl + CE_EPI_PLANE16 + fr * 144 + (dh * 4 + fq) * 16);
                        half_t* o = kf16 + ((((size_t)head * (m_pad >> 4) + (m >> 4)) * 2 + dh) * 64 + lane) * 8;
                        __builtin_nontemporal_store(hi, reinterpret_cast<half8*>(o));
                        __builtin_nontemporal_store(lo, reinterpret_cast<half8*>(o + kv_plane));
                    }
                } else {
                    // K features -> kf16[head][16-row tile of the PACKED row space][lane = fq*16 + key%16][8 dims fq*8..]: the MFMA
                    // A-fragment order the attention kernel DMAs straight into LDS; a pair's keys are consecutive tiles of one head
                    // (pairs start at multiples of 16 rows). One store instruction = one whole 1 KiB fragment tile.
                    const int head0 = (nb - hidden) >> 5;          // this wave's 64 features = heads head0, head0+1
                    const int m = mb + j * 16;
#pragma unroll
                    for (int hl = 0; hl < 2; ++hl) {
                        const half8 hi = *reinterpret_cast<const half8*>(wl + fr * 144 + (hl * 4 + fq) * 16);
                        const half8 lo = *reinterpret_cast<const half8*>(wl + CE_EPI_PLANE16 + fr * 144 + (hl * 4 + fq) * 16);
                        half_t* o = kf16 + (((size_t)(head0 + hl) * (m_pad >> 4) + (m >> 4)) * 64 + lane) * 8;
                        __builtin_nontemporal_store(hi, reinterpret_cast<half8*>(o));
                        __builtin_nontemporal_store(lo, reinterpret_cast<half8*>(o + kv_plane));
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        } else {
            // EPI_QKV, V features: one fp16 plane of [64 features][32 tokens] at a time (rows 80 B), then
            // vf16[head][16-row tile of the PACKED row space][d half][lane = fq*16 + d%16][4 key slots = rows fq*4..+4 of the
            // tile]. The attention kernel reads a lane's 8 B of two adjacent tiles as one MFMA A fragment: 8 key slots in the
            // order in which the S^T accumulators of the two key tiles sit in a lane's registers, so P never leaves registers.
            // Tiles (not 32-row blocks) are the unit so that a pair may start at any multiple of 16 rows.
            // 64-wide heads (EPI_QKV64): the 64 features are one head's four 16-dim quarters, a tile is [d quarter][lane][4 key slots] =
            // 2 KiB per (head, tile) and plane; the store pattern is the same with the tile stride doubled.
            const int head0 = EPI == EPI_QKV64 ? (nb - 2 * hidden) >> 6 : (nb - 2 * hidden) >> 5;
#pragma unroll
            for (int kl = 0; kl < 2; ++kl) {
                const int m = mb + kl * 32;
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v = acc[i][kl * 2 + jj][r] + (r == 0 ? bv[i].x : r == 1 ? bv[i].y : r == 2 ? bv[i].z : bv[i].w);
                                const half_t hi = (half_t)v;
                                *reinterpret_cast<half_t*>(wl + (i * 16 + fq * 4 + r) * 80 + (jj * 16 + fr) * 2) =
                                    pl == 0 ? hi : (half_t)(v - (float)hi);
                            }
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int hl = it >> 1, dh = it & 1;            // head, d half
                        const char* rowp = wl + (hl * 32 + dh * 16 + fr) * 80 + fq * 8;
                        const half4 h0 = *reinterpret_cast<const half4*>(rowp), h1 = *reinterpret_cast<const half4*>(rowp + 32);
                        half_t* o = EPI == EPI_QKV64
                                        ? vf16 + ((((size_t)head0 * (m_pad >> 4) + (m >> 4)) * 4 + it) * 64 + lane) * 4 + (pl ? kv_plane : 0)
                                        : vf16 + ((((size_t)(head0 + hl) * (m_pad >> 4) + (m >> 4)) * 2 + dh) * 64 + lane) * 4 + (pl ? kv_plane : 0);
                        __builtin_nontemporal_store(h0, reinterpret_cast<half4*>(o));
                        __builtin_nontemporal_store(h1, reinterpret_cast<half4*>(o + (EPI == EPI_QKV64 ? 1024 : 512)));   // the next 16-row tile
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (!has_next) break;
        // next tile: its steps 0 and 1 are resident (waited above); the stage this epilogue used is refilled by CE_ISSUE(2)
        // in the coming I-part, so every wave must be done reading it first
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        CE_BAR
        work += n_slots;
        w_cur = w_nxt;
        x_cur = x_nxt;
        sbase = (sbase + nt) % 3;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // clamped tail re-loads of the last tile: retire them before exit
}

// ---- LayerNorm helpers: one wave per token row of `hidden` floats (hidden % 64 == 0, <= 1024) --------------
template <int PER>
__device__ __forceinline__ void wave_layernorm(float (&v)[PER], const float* __restrict__ g, const float* __restrict__ b,
                                               int hidden, float eps, int lane, half_t* __restrict__ o16) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)hidden;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { const float d = v[i] - mean; q += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)hidden + eps);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = lane + i * 64;
        const float y = (v[i] - mean) * rstd * g[c] + b[c];
        const half_t hi = (half_t)y;
        o16[SPLIT_IDX(c)] = hi;
        o16[SPLIT_IDX(c) + 32] = (half_t)(y - (float)hi);
    }
}

// ---- packing: pair p owns len_p rounded up to 16 rows of the attention space and to g rows of the GEMM row space; offsets by one
// block-wide scan, then the maps of the GEMM rows.
// The ONE place that reads the caller's lens: a length is clamped to [1, L_in] (L_in = the caller's padded length, not the attention
// length class it was rounded up to: tokens past L_in do not exist) and written to clen, which attention and the pooling heads read.
// Two prefix sums: pair_off over the lengths rounded up to 16 (attention space), row_off over the lengths rounded up to g = 4 or 16
// (GEMM row space; g = 16: the same numbers).
__global__ __launch_bounds__(1024) void ce_pack_scan_kernel(const int32_t* __restrict__ lens, int P, int L_in, int g, int32_t* __restrict__ clen,
                                                             int32_t* __restrict__ pair_off, int32_t* __restrict__ row_off,
                                                             int32_t* __restrict__ m_packed) {
    __shared__ int part[1024], part_g[1024];
    const int tid = threadIdx.x;
    const int per = (P + 1023) / 1024;
    const int b = tid * per, e = min(P, b + per);
    int s = 0, sg = 0;
    for (int p = b; p < e; ++p) {
        const int len = max(1, min(lens[p], L_in));
        s += (len + 15) & ~15;
        sg += (len + g - 1) & ~(g - 1);
    }
    part[tid] = s;
    part_g[tid] = sg;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0, vg = tid >= o ? part_g[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        part_g[tid] += vg;
        __syncthreads();
    }
    int off = part[tid] - s, off_g = part_g[tid] - sg;
    for (int p = b; p < e; ++p) {
        const int len = max(1, min(lens[p], L_in));
        clen[p] = len;
        pair_off[p] = off;
        row_off[p] = off_g;
        off += (len + 15) & ~15;
        off_g += (len + g - 1) & ~(g - 1);
    }
    if (tid == 1023) { pair_off[P] = part[1023]; row_off[P] = part_g[1023]; m_packed[0] = part_g[1023]; }
}

// The maps of the GEMM row space: owning pair and attention row of every row (-1 from row_off[P] up to the allocated rows)
__global__ void ce_pack_rows_kernel(const int32_t* __restrict__ pair_off, const int32_t* __restrict__ row_off, int P, int L, int64_t rows_total,
                                    int32_t* __restrict__ row_pair, int32_t* __restrict__ row_att) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows_total && i >= row_off[P]) row_pair[i] = row_att[i] = -1;
    if (i >= (int64_t)P * L) return;
    const int p = (int)(i / L), t = (int)(i % L);
    if (t < row_off[p + 1] - row_off[p]) {
        row_pair[row_off[p] + t] = p;
        row_att[row_off[p] + t] = pair_off[p] + t;
    }
}

template <int PER>
__global__ __launch_bounds__(256) void ce_embed_ln_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ tt,
                                                           const float* __restrict__ word, const float* __restrict__ pos,
                                                           const float* __restrict__ type, const float* __restrict__ g,
                                                           const float* __restrict__ b, const int32_t* __restrict__ m_packed,
                                                           const int32_t* __restrict__ row_pair, const int32_t* __restrict__ pair_off,
                                                           int L, int hidden, int vocab, int max_pos, float eps, half_t* __restrict__ x16) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m_packed[0]) return;
    const int pr = row_pair[row];
    const int p = (int)row - pair_off[pr];                    // position inside the pair (< L: the rounded length never exceeds L)
    // a real token sits below seq_len <= max_pos; the pad rows behind a length that is no multiple of 16 may lie past the position
    // table when max_pos is no multiple of 16 either: they take its last row (their values are never read, but must be finite)
    const int pp = min(p, max_pos - 1);
    const size_t src = (size_t)pr * L + p;
    int id = ids[src];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const int ty = tt[src] != 0;
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = lane + i * 64;
        v[i] = word[(size_t)id * hidden + c] + type[(size_t)ty * hidden + c] + pos[(size_t)pp * hidden + c];
    }
    wave_layernorm<PER>(v, g, b, hidden, eps, lane, x16 + row * 2 * hidden);
}

template <int PER>
__global__ __launch_bounds__(256) void ce_layernorm_kernel(const float* __restrict__ y32, const float* __restrict__ g,
                                                            const float* __restrict__ b, const int32_t* __restrict__ m_packed,
                                                            int hidden, float eps, half_t* __restrict__ x16) {
    const int lane = threadIdx.x & 63;
    const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= m_packed[0]) return;
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) v[i] = y32[tok * hidden + lane + i * 64];
    wave_layernorm<PER>(v, g, b, hidden, eps, lane, x16 + tok * 2 * hidden);
}

// ---- attention: d_head must be 32. One block per (head, pair); every wave owns QB consecutive 16-query blocks.
// K and V of the (pair, head) arrive in LDS by LDS-DMA, already in MFMA fragment order (written that way by the QKV
// epilogue) as 1 KiB tiles of 16 packed rows: a K fragment is one conflict-free ds_read_b128 at lane*16, a V fragment two
// ds_read_b64 at lane*8 (the lane's key slots of two adjacent tiles); both are shared by all waves of the block.
// All operands are split fp16 (hi + lo plane): S and P.V are 3 MFMAs each. S is computed TRANSPOSED (A = K rows,
// B = Q rows): the accumulator lane (fr, fq) then holds query fr x keys fq*4..+4, which IS the B-operand layout of the
// next MFMA if the 32 k-slots of a key block are numbered (fq, e) -> key fq*4 + e (e < 4) | 16 + fq*4 + e - 4: V is
// stored in that slot order, so P goes registers -> MFMA without touching LDS. Online (flash-style) softmax over
// 32-key blocks in the exp2 domain; key blocks past the pair's length are skipped, the boundary block is masked.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t ce_pk(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
}
__device__ __forceinline__ float ce_trunc10(float e) {     // e with the mantissa cut to 10 bits: exactly a fp16 value
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, e) & 0xFFFFE000u);
}
__device__ __forceinline__ void ce_dma_at(const half_t* __restrict__ g, char* lds_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_uniform, 16, 0, 0);
}

// MX = true (the hi16 + lo8 forward, ce_mx.h): Q arrives in the same fragment order as K (q16 = qf16[head][16-row tile][lane][8], lo
// plane kv_plane further) and the context leaves in the image layout of the out-projection's token operand (ctx16 = ctx8 bytes).
// DIRECT (the [CLS]-only last layer: one 16-query block per pair): ONE wave per (head, pair) reads the K / V fragment tiles straight
// from global memory - every tile is used by that one wave, so staging it in LDS only costs a 64-KiB allocation per workgroup.
template <int QB, bool MX = false, bool DIRECT = false>
__global__ __launch_bounds__(1024) void ce_attention_kernel(const half_t* __restrict__ q16,
                                                             const half_t* __restrict__ kf16, const half_t* __restrict__ vf16,
                                                             size_t kv_plane, const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ pair_off, const int32_t* __restrict__ row_off,
                                                             int L, int hidden, int heads, int m_pad, half_t* __restrict__ ctx16,
                                                             int max_qblocks = 1 << 20) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
    const int head = blockIdx.x, pair = blockIdx.y;
    const int len = max(1, min(lens[pair], L));
    const int fr = lane & 15, fq = lane >> 4;
    const int po = pair_off[pair], Lp = pair_off[pair + 1] - po;     // this pair's rows in attention space: len rounded up to 16
    // its rows in the GEMM row space, where the context goes: len rounded up to 4 or 16. Q, K and V of the slots [Lr, Lp) of the
    // pair's last tile were written by no GEMM of this forward when Lr < Lp: they hold whatever an earlier call left there.
    const int ro = row_off[pair], Lr = row_off[pair + 1] - ro;
    const int nt = Lp >> 4;                                           // the pair's 16-row tiles; an odd count leaves the second
    const int nkb = (len + 31) >> 5;                                  // half of the last 32-key block outside the pair (masked)
    const size_t plane_b = (size_t)L * 64;                            // bytes of one K (or V) plane of this (pair, head)
    const size_t t0 = ((size_t)head * (m_pad >> 4) + (po >> 4)) * 512;                      // first tile of this (head, pair), in halfs
    // fragment reads below address tile c of a plane at byte c * 1024 + (lane's offset): the same bytes in LDS and in global memory
    const char* const k_hi = DIRECT ? reinterpret_cast<const char*>(kf16 + t0) : smem;
    const char* const k_lo = DIRECT ? reinterpret_cast<const char*>(kf16 + t0 + kv_plane) : smem + plane_b;
    const char* const v_hi = DIRECT ? reinterpret_cast<const char*>(vf16 + t0) : smem + 2 * plane_b;
    const char* const v_lo = DIRECT ? reinterpret_cast<const char*>(vf16 + t0 + kv_plane) : smem + 3 * plane_b;
    if (!DIRECT) {
        char* const sk_hi = smem;
        char* const sk_lo = smem + plane_b;
        char* const sv_hi = smem + 2 * plane_b;
        char* const sv_lo = smem + 3 * plane_b;
        const size_t g0 = (((size_t)head * (m_pad >> 4) + (po >> 4)) * 64 + lane) * 8;   // K and V tiles are both 1 KiB per plane
        for (int c = wv; c < nt; c += nwaves) {
            ce_dma_at(kf16 + g0 + (size_t)c * 512, sk_hi + c * 1024);
            ce_dma_at(kf16 + g0 + kv_plane + (size_t)c * 512, sk_lo + c * 1024);
            ce_dma_at(vf16 + g0 + (size_t)c * 512, sv_hi + c * 1024);
            ce_dma_at(vf16 + g0 + kv_plane + (size_t)c * 512, sv_lo + c * 1024);
        }
        // an odd tile count leaves the second half of the last 32-key block outside the pair: P is 0 there (masked keys), V must be
        // finite (0 x NaN = NaN) - the never-staged tile is zeroed once instead of selecting zeros at every fragment read. DIRECT
        // would read the next pair's rows or stale slack there, which may hold anything: it selects zeros for that tile instead.
        if ((nt & 1) && wv == 0) {
            *reinterpret_cast<u32x4*>(sv_hi + nt * 1024 + lane * 16) = (u32x4){0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(sv_lo + nt * 1024 + lane * 16) = (u32x4){0u, 0u, 0u, 0u};
        }
    }
    const size_t row0 = (size_t)po;
    const int qb0 = wv * QB;
    // max_qblocks: only the first max_qblocks 16-query blocks of a pair are computed (the last layer of a classifier needs the [CLS]
    // row alone; the other waves still help with the K / V DMA)
    const bool has_rows = qb0 * 16 < Lp && qb0 < max_qblocks;         // waves past the pair's rows only helped with the DMA
    // B operand = Q rows (query fr of block b, dims 8*fq..+8)
    half8 qh[QB], ql[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        // split-row layout: a head's 32 dims are one K group = [hi 32 | lo 32] halfs
        const int qb = (qb0 + b) * 16 < Lp ? qb0 + b : qb0;           // a block past the pair's rows is computed but not stored
        if (MX) {
            const half_t* qp = q16 + (((size_t)head * (m_pad >> 4) + (po >> 4) + qb) * 64 + lane) * 8;
            qh[b] = *reinterpret_cast<const half8*>(qp);
            ql[b] = *reinterpret_cast<const half8*>(qp + kv_plane);
        } else {
            const half_t* qp = q16 + (row0 + qb * 16 + fr) * (2 * hidden) + head * 64 + fq * 8;
            qh[b] = *reinterpret_cast<const half8*>(qp);
            ql[b] = *reinterpret_cast<const half8*>(qp + 32);
        }
    }
    f32x4 c0[QB], c1[QB];
    float mrun[QB], lsum[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        c0[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        c1[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mrun[b] = -INFINITY;
        lsum[b] = 0.f;
    }
    const float cs = (float)(0.17677669529663687 * 1.4426950408889634);    // 32^-0.5 * log2(e)
    if (!DIRECT) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // The stale V slots of the last tile (keys Lr .. Lp - 1: P = 0 there, V must be finite) are zeroed once, by the wave whose DMA
        // staged that tile, after its own wait above has landed it. They are the whole slot groups fq >= (Lr & 15) >> 2: one
        // contiguous run per d half of the tile ([d half][fq * 16 + d % 16][4 slots], 128 B per group); lane -> the tile's 16-B piece.
        if (MX && Lr < Lp && wv == (nt - 1 < nwaves ? nt - 1 : nt - 1 - nwaves) && ((lane & 31) >> 3) >= ((Lr & 15) >> 2)) {   // nt <= 2 nwaves
            char* const sv = smem + 2 * plane_b + (nt - 1) * 1024 + lane * 16;
            *reinterpret_cast<u32x4*>(sv) = (u32x4){0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(sv + plane_b) = (u32x4){0u, 0u, 0u, 0u};
        }
        __syncthreads();
    }
    if (!has_rows) return;
    // v_med3_f32(a, b, +inf) = max(a, b): fmaxf on MFMA results costs a canonicalising v_max x, x per input (15 instructions for 8
    // scores where 7 do); the +inf sits in a scalar register the compiler cannot fold
    float ce_inf;
    asm volatile("s_mov_b32 %0, 0x7f800000" : "=s"(ce_inf));
#define CE_MAX2(a_, b_) __builtin_amdgcn_fmed3f(a_, b_, ce_inf)
    // one 32-key block; EDGE (the pair's last block only: the loop is peeled) masks the keys past the pair's length
    auto key_block = [&](const int kb, auto edge_c) {
        constexpr bool EDGE = decltype(edge_c)::value;
        const int fo = kb * 2048 + lane * 16;
        const half8 k0h = *reinterpret_cast<const half8*>(k_hi + fo), k1h = *reinterpret_cast<const half8*>(k_hi + fo + 1024);
        const half8 k0l = *reinterpret_cast<const half8*>(k_lo + fo), k1l = *reinterpret_cast<const half8*>(k_lo + fo + 1024);
        // V fragment = the lane's 4 key slots of tile 2kb | of tile 2kb+1 (tile = [d half][lane][4 slots], 512 B per half); tile 2kb+1
        // of an odd-count pair lies outside the pair under P = 0: zeros in LDS, and DIRECT selects zeros (that memory belongs to the
        // next pair or is stale slack: a non-finite value there would turn this pair's context into NaN)
        const int vo = kb * 2048 + lane * 8;
        half4 a0h = *reinterpret_cast<const half4*>(v_hi + vo), a1h = *reinterpret_cast<const half4*>(v_hi + vo + 512);
        half4 a0l = *reinterpret_cast<const half4*>(v_lo + vo), a1l = *reinterpret_cast<const half4*>(v_lo + vo + 512);
        half4 b0h = {}, b1h = {}, b0l = {}, b1l = {};
        if (!(DIRECT && EDGE && (nt & 1))) {
            b0h = *reinterpret_cast<const half4*>(v_hi + vo + 1024);
            b1h = *reinterpret_cast<const half4*>(v_hi + vo + 1536);
            b0l = *reinterpret_cast<const half4*>(v_lo + vo + 1024);
            b1l = *reinterpret_cast<const half4*>(v_lo + vo + 1536);
        }
        // DIRECT has no staged copy to zero: the lane's slot group (4 keys from fq * 4 on in each tile) past the pair's GEMM rows is
        // stale, and selected to zero here (the LDS form zeroed those groups after staging)
        if (DIRECT && EDGE && MX) {
            if (kb * 32 + fq * 4 >= Lr) a0h = a1h = a0l = a1l = (half4){};
            if (kb * 32 + 16 + fq * 4 >= Lr) b0h = b1h = b0l = b1l = (half4){};
        }
        const half8 v0h = __builtin_shufflevector(a0h, b0h, 0, 1, 2, 3, 4, 5, 6, 7), v1h = __builtin_shufflevector(a1h, b1h, 0, 1, 2, 3, 4, 5, 6, 7);
        const half8 v0l = __builtin_shufflevector(a0l, b0l, 0, 1, 2, 3, 4, 5, 6, 7), v1l = __builtin_shufflevector(a1l, b1l, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
            z0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0l, qh[b], z0, 0, 0, 0);
            z1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1l, qh[b], z1, 0, 0, 0);
            z0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0h, ql[b], z0, 0, 0, 0);
            z1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1h, ql[b], z1, 0, 0, 0);
            z0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0h, qh[b], z0, 0, 0, 0);
            z1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1h, qh[b], z1, 0, 0, 0);
            // lane (fr, fq): z0[r] = S[query fr][key kb*32 + fq*4 + r], z1[r] = same + 16
            if (EDGE) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (kb * 32 + fq * 4 + r >= len) z0[r] = -INFINITY;
                    if (kb * 32 + 16 + fq * 4 + r >= len) z1[r] = -INFINITY;
                }
            }
            float mx = CE_MAX2(CE_MAX2(CE_MAX2(z0[0], z0[1]), CE_MAX2(z0[2], z0[3])), CE_MAX2(CE_MAX2(z1[0], z1[1]), CE_MAX2(z1[2], z1[3])));
            // lane ^ 16 and lane ^ 32 by v_permlane16_swap / v_permlane32_swap of (mx, copy of mx): after the swap the two registers hold
            // the lane's own value and its partner's (tools/permlane_probe.hip) - no LDS round trip on the softmax's critical path. The
            // instructions are issued by hand: through the builtins this compiler folds the swap's second result into its first when both
            // feed one expression, and the maximum silently becomes "the value of lane group 0".
            {
                float cp = mx;
                asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(mx), "+v"(cp));
                mx = CE_MAX2(mx, cp);
                cp = mx;
                asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(mx), "+v"(cp));
                mx = CE_MAX2(mx, cp);
            }
            const float mnew = CE_MAX2(mrun[b], mx);                // finite: key 0 is always real
            const float alpha = __builtin_amdgcn_exp2f((mrun[b] - mnew) * cs);
            mrun[b] = mnew;
            const float off = -mnew * cs;
            float e[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                e[r] = __builtin_amdgcn_exp2f(fmaf(z0[r], cs, off));
                e[4 + r] = __builtin_amdgcn_exp2f(fmaf(z1[r], cs, off));
            }
            lsum[b] = lsum[b] * alpha + (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
#pragma unroll
            for (int r = 0; r < 4; ++r) { c0[b][r] *= alpha; c1[b][r] *= alpha; }
            float eh[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) eh[r] = ce_trunc10(e[r]);
            const u32x4 ph_u = {ce_pk(eh[0], eh[1]), ce_pk(eh[2], eh[3]), ce_pk(eh[4], eh[5]), ce_pk(eh[6], eh[7])};
            const u32x4 pl_u = {ce_pk(e[0] - eh[0], e[1] - eh[1]), ce_pk(e[2] - eh[2], e[3] - eh[3]),
                                ce_pk(e[4] - eh[4], e[5] - eh[5]), ce_pk(e[6] - eh[6], e[7] - eh[7])};
            const half8 ph = __builtin_bit_cast(half8, ph_u), pl = __builtin_bit_cast(half8, pl_u);
            // ctx^T[d][q] += V^T[d][key] P[q][key]: A = V fragment (row d), B = P (col q = fr)
            c0[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(v0l, ph, c0[b], 0, 0, 0);
            c1[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(v1l, ph, c1[b], 0, 0, 0);
            c0[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(v0h, pl, c0[b], 0, 0, 0);
            c1[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(v1h, pl, c1[b], 0, 0, 0);
            c0[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(v0h, ph, c0[b], 0, 0, 0);
            c1[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(v1h, ph, c1[b], 0, 0, 0);
        }
    };
    for (int kb = 0; kb + 1 < nkb; ++kb) key_block(kb, std::false_type{});
    key_block(nkb - 1, std::true_type{});
#undef CE_MAX2
    // lane (fr, fq): c0[r] = ctx[query fr][d = fq*4 + r], c1[r] = d + 16; the row sum is spread over the 4 fq lanes
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        float l = lsum[b];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        if ((qb0 + b) * 16 >= Lp || qb0 + b >= max_qblocks) break;
        if (MX) {
            // the context goes to the pair's GEMM rows; queries past them (stale Q rows of the last tile: a query is one MFMA column,
            // and the maximum and the sum above stay inside it) have no row there
            if ((qb0 + b) * 16 + fr >= Lr) continue;
            // K-step = head; c0 = dims 4fq..4fq+3 (MFMA j = 0), c1 = 16 + the same (j = 1); lane half h = fq & 1, position 4 (fq >> 1) + r
            const int64_t mrow = (int64_t)ro + (qb0 + b) * 16 + fr;
            char* img = reinterpret_cast<char*>(ctx16) + mx_img_base(mrow, head * 32, hidden >> 5) + (int)(mrow & 127) * 16 + (fq >> 1) * 8;
            mx_u2 h0, h1;
            unsigned l0, l1;
            mx_split4(c0[b][0] * inv, c0[b][1] * inv, c0[b][2] * inv, c0[b][3] * inv, h0, l0);
            mx_split4(c1[b][0] * inv, c1[b][1] * inv, c1[b][2] * inv, c1[b][3] * inv, h1, l1);
            *reinterpret_cast<mx_u2*>(img + (fq & 1) * MX_B_PLANE) = h0;
            *reinterpret_cast<mx_u2*>(img + (2 + (fq & 1)) * MX_B_PLANE) = h1;
            *reinterpret_cast<mx_u2*>(img + (4 + (fq & 1)) * MX_B_PLANE) = (mx_u2){l0, l1};
            continue;
        }
        half_t* o = ctx16 + (row0 + (qb0 + b) * 16 + fr) * (2 * hidden) + head * 64 + fq * 4;
        store_split4(o, 32, c0[b][0] * inv, c0[b][1] * inv, c0[b][2] * inv, c0[b][3] * inv);
        store_split4(o + 16, 32, c1[b][0] * inv, c1[b][1] * inv, c1[b][2] * inv, c1[b][3] * inv);
    }
}

// ---- attention for d_head = 64 (split-fp16 forward only). The scheme of ce_attention_kernel: one workgroup per (head, pair), two
// 16-query blocks per wave, S transposed so that P stays in registers, online softmax over 32-key blocks in the exp2 domain, hi + lo
// operands with three products per MFMA position, the edge block masked. What differs: S chains two 16x16x32 MFMAs over the head's two
// 32-dim halves per product, P.V fills four 16-dim accumulators per query block, the scale is 64^-0.5 * log2(e), and a 16-row tile is
// 2 KiB per plane (K: [dim half][lane][8 dims], V: [d quarter][lane][4 key slots]; written by the EPI_QKV64 epilogue).
// The four planes cost 512 B per key: the length classes up to 256 are staged whole in LDS (128 KiB), classes 384 and 512 do not
// fit in 160 KiB and read the same fragment bytes straight from global memory (DIRECT; every tile is read by all waves of the
// (head, pair), out of L2). DIRECT waves share nothing, so a (head, pair) is split over blockIdx.z into workgroups of 8 waves (256
// queries each): 16 waves in one workgroup would cap the kernel at 128 VGPRs, which it does not fit without scratch. All forms consume the keys in the same 32-key-block order with the same instructions, so a sequence's result does
// not depend on its length class.
//
// STREAM (the classes above 512, up to 8192 keys): the DIRECT geometry - grid (heads, P, L / 256), 8 waves = 256 queries of one
// (head, pair) - but the workgroup's eight waves share every K / V fragment: the pair's 32-key blocks (K hi | K lo | V hi | V lo,
// 4 KiB each = 16 KiB) pass through a ring of CE_A64_RING = 4 LDS slots, filled by the LDS-DMA of the resident form. One block
// per stage: wave w copies tile (w & 1) of plane (w >> 1), two 1-KiB DMAs per block. Per block: the wave waits for ITS two DMAs
// of block kb by a counted vmcnt (the blocks staged after it stay in flight), one workgroup barrier makes every wave's part of
// block kb visible and frees the slot of block kb - 1 (all its fragment reads were consumed by MFMAs before the barrier), the wave
// stages block kb + 3 into that slot and then computes block kb. Three blocks (48 KiB) are in flight under a block's 48 MFMAs
// per wave; a shallower ring leaves two, a deeper one only adds cases to the counted wait. One block per stage keeps a stage at the 32-key
// step of the online softmax and costs one barrier per 48 MFMAs. Ring = 4 x 16 KiB = 64 KiB of the CU's 160 KiB. The compiler
// reports 152 VGPRs, no scratch, 3 waves per SIMD for this form (DIRECT: 152, resident: 153), so the registers, not the LDS, hold a
// CU to ONE 8-wave workgroup in both forms above class 256; the ring could be 2.5 x as deep at no cost in occupancy, the measured
// gain did not ask for it. L2 reads of K / V per (head, pair) drop from 8 x to 1 x per workgroup.
// Three things this form alone must get right: (1) a workgroup whose 256 queries all lie past the pair's rows leaves before its
// first barrier (uniform), but a WAVE past the rows of a live workgroup keeps staging and reaches every barrier - it only skips
// the arithmetic; (2) tile nt of a pair with an odd tile count (second half of the last block) is never copied: its V slots are
// zeroed in the ring, as the resident form zeroes them, because P = 0 there and 0 x NaN would poison the context (its K slots are
// whatever the ring held: those scores are overwritten by -inf); (3) only the pair's own nkb blocks are staged, never L / 32.
#define CE_A64_RESIDENT 0
#define CE_A64_DIRECT 1
#define CE_A64_STREAM 2
#define CE_A64_RING 4                                                  // LDS slots of the streamed form (a power of two)
#define CE_A64_SLOT 16384                                              // bytes of one slot: one 32-key block of the four planes
template <int MODE>
__global__ __launch_bounds__(512) void ce_attention64_kernel(const half_t* __restrict__ q16, const half_t* __restrict__ kf16,
                                                                              const half_t* __restrict__ vf16, size_t kv_plane,
                                                                              const int32_t* __restrict__ lens, const int32_t* __restrict__ pair_off,
                                                                              int L, int hidden, int m_pad, half_t* __restrict__ ctx16) {
    constexpr bool DIRECT = MODE == CE_A64_DIRECT, STREAM = MODE == CE_A64_STREAM;
    constexpr int QB = 2;                                             // 16-query blocks per wave, in every length class
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
    const int head = blockIdx.x, pair = blockIdx.y;
    const int len = max(1, min(lens[pair], L));
    const int fr = lane & 15, fq = lane >> 4;
    const int po = pair_off[pair], Lp = pair_off[pair + 1] - po;     // this pair's packed rows: len rounded up to 16
    const int nt = Lp >> 4;                                           // the pair's 16-row tiles; an odd count leaves the second
    const int nkb = (len + 31) >> 5;                                  // half of the last 32-key block outside the pair (masked)
    if (STREAM && (int)blockIdx.z * 256 >= Lp) return;                // the whole workgroup, before its first barrier
    // bytes of one K (or V) plane of this (pair, head); STREAM: of one ring slot. L <= 8192: L * 128 <= 2^20, and the block offsets
    // kb * 4096 below stay under 2^20 as well (kb < 256), so 32-bit byte offsets hold in every form.
    const size_t plane_b = STREAM ? 4096 : (size_t)L * 128;
    const size_t t0 = ((size_t)head * (m_pad >> 4) + (po >> 4)) * 1024;                     // first tile of this (head, pair), in halfs
    // fragment reads below address tile c of a plane at byte c * 2048 + (lane's offset): the same bytes in LDS and in global memory
    // (STREAM: tiles 2kb and 2kb + 1 sit at bytes 0 and 2048 of the planes of slot kb % CE_A64_RING)
    const char* const k_hi = DIRECT ? reinterpret_cast<const char*>(kf16 + t0) : smem;
    const char* const k_lo = DIRECT ? reinterpret_cast<const char*>(kf16 + t0 + kv_plane) : smem + plane_b;
    const char* const v_hi = DIRECT ? reinterpret_cast<const char*>(vf16 + t0) : smem + 2 * plane_b;
    const char* const v_lo = DIRECT ? reinterpret_cast<const char*>(vf16 + t0 + kv_plane) : smem + 3 * plane_b;
    // STREAM: this wave's share of every block = tile s_tl of plane s_pl (0 K hi, 1 K lo, 2 V hi, 3 V lo)
    const int s_pl = wv >> 1, s_tl = wv & 1;
    const half_t* const s_src = ((s_pl & 2) ? vf16 : kf16) + t0 + ((s_pl & 1) ? kv_plane : 0) + (size_t)s_tl * 1024 + (size_t)lane * 8;
    const int s_dst = s_pl * 4096 + s_tl * 2048;
    const bool s_skip_last = (nt & 1) && s_tl;                        // this wave's tile of the last block is tile nt: outside the pair
    auto stream_stage = [&](const int blk) {
        char* const d = smem + (blk & (CE_A64_RING - 1)) * CE_A64_SLOT + s_dst;
        if (s_skip_last && blk == nkb - 1) {
            if (s_pl & 2) {
                *reinterpret_cast<u32x4*>(d + lane * 16) = (u32x4){0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4*>(d + 1024 + lane * 16) = (u32x4){0u, 0u, 0u, 0u};
            }
            return;
        }
        ce_dma_at(s_src + (size_t)blk * 2048, d);
        ce_dma_at(s_src + (size_t)blk * 2048 + 512, d + 1024);
    };
    if (STREAM)
        for (int blk = 0; blk < CE_A64_RING - 1 && blk < nkb; ++blk) stream_stage(blk);
    if (MODE == CE_A64_RESIDENT) {
        char* const sk_hi = smem;
        char* const sk_lo = smem + plane_b;
        char* const sv_hi = smem + 2 * plane_b;
        char* const sv_lo = smem + 3 * plane_b;
        const size_t g0 = t0 + (size_t)lane * 8;                      // a tile is two 1-KiB pieces per plane
        for (int c = wv; c < nt; c += nwaves)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const size_t g = g0 + (size_t)c * 1024 + j * 512;
                const int s = c * 2048 + j * 1024;
                ce_dma_at(kf16 + g, sk_hi + s);
                ce_dma_at(kf16 + g + kv_plane, sk_lo + s);
                ce_dma_at(vf16 + g, sv_hi + s);
                ce_dma_at(vf16 + g + kv_plane, sv_lo + s);
            }
        // an odd tile count leaves the second half of the last 32-key block outside the pair: P is 0 there (masked keys), V must be
        // finite (0 x NaN = NaN). The never-staged tile is zeroed once; DIRECT selects zeros for it at the fragment read, because
        // that memory belongs to the next pair or is stale slack.
        if ((nt & 1) && wv == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                *reinterpret_cast<u32x4*>(sv_hi + nt * 2048 + j * 1024 + lane * 16) = (u32x4){0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4*>(sv_lo + nt * 2048 + j * 1024 + lane * 16) = (u32x4){0u, 0u, 0u, 0u};
            }
        }
    }
    const size_t row0 = (size_t)po;
    const int qb0 = ((DIRECT || STREAM ? (int)blockIdx.z * nwaves : 0) + wv) * QB;
    const bool has_rows = qb0 * 16 < Lp;                              // waves past the pair's rows only helped with the DMA
    // B operand = Q rows (query fr of block b, dims half*32 + 8*fq..+8). Split-row layout: a head's 64 dims are two K groups of
    // [hi 32 | lo 32] halfs
    half8 qh[QB][2], ql[QB][2];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        // a block past the pair's rows is computed but not stored (a STREAM wave without rows computes nothing: it reads block 0)
        const int qb = (qb0 + b) * 16 < Lp ? qb0 + b : (STREAM && !has_rows ? 0 : qb0);
        const half_t* qp = q16 + (row0 + qb * 16 + fr) * (2 * hidden) + head * 128 + fq * 8;
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
            qh[b][dh] = *reinterpret_cast<const half8*>(qp + dh * 64);
            ql[b][dh] = *reinterpret_cast<const half8*>(qp + dh * 64 + 32);
        }
    }
    f32x4 cx[QB][4];
    float mrun[QB], lsum[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
#pragma unroll
        for (int dq = 0; dq < 4; ++dq) cx[b][dq] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mrun[b] = -INFINITY;
        lsum[b] = 0.f;
    }
    const float cs = (float)(0.125 * 1.4426950408889634);             // 64^-0.5 * log2(e)
    if (STREAM) {
        // Q is the kernel's only ordinary load: it is waited for HERE (the empty statements read the registers), before the loop, so
        // that no wait for it lands between the counted waits of the ring and drains them
#pragma unroll
        for (int b = 0; b < QB; ++b)
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) asm volatile("" ::"v"(qh[b][dh]), "v"(ql[b][dh]));
    }
    if (MODE == CE_A64_RESIDENT) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (!STREAM && !has_rows) return;                                 // STREAM: such a wave stays for the staging and the barriers
    float ce_inf;                                                     // see ce_attention_kernel: max by v_med3_f32(a, b, +inf)
    asm volatile("s_mov_b32 %0, 0x7f800000" : "=s"(ce_inf));
#define CE_MAX2(a_, b_) __builtin_amdgcn_fmed3f(a_, b_, ce_inf)
    // one 32-key block = tiles 2kb and 2kb+1; EDGE (the pair's last block only: the loop is peeled) masks the keys past the length
    auto key_block = [&](const int kb, auto edge_c) {
        constexpr bool EDGE = decltype(edge_c)::value;
        const int bo = STREAM ? (kb & (CE_A64_RING - 1)) * CE_A64_SLOT : kb * 4096;     // the block's byte offset in each plane
        const int fo = bo + lane * 16;
        half8 kh[2][2], kl[2][2];                                     // [tile][dim half]
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                kh[t][dh] = *reinterpret_cast<const half8*>(k_hi + fo + t * 2048 + dh * 1024);
                kl[t][dh] = *reinterpret_cast<const half8*>(k_lo + fo + t * 2048 + dh * 1024);
            }
        // V fragment of d quarter dq = the lane's 4 key slots of tile 2kb | of tile 2kb+1. Tile 2kb+1 of an odd-count pair lies outside
        // the pair under P = 0: zeros in LDS, and DIRECT selects zeros.
        const int vo = bo + lane * 8;
        half8 vh[4], vl[4];
#pragma unroll
        for (int dq = 0; dq < 4; ++dq) {
            const half4 ah = *reinterpret_cast<const half4*>(v_hi + vo + dq * 512), al = *reinterpret_cast<const half4*>(v_lo + vo + dq * 512);
            half4 bh = {}, bl = {};
            if (!(DIRECT && EDGE && (nt & 1))) {
                bh = *reinterpret_cast<const half4*>(v_hi + vo + 2048 + dq * 512);
                bl = *reinterpret_cast<const half4*>(v_lo + vo + 2048 + dq * 512);
            }
            vh[dq] = __builtin_shufflevector(ah, bh, 0, 1, 2, 3, 4, 5, 6, 7);
            vl[dq] = __builtin_shufflevector(al, bl, 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
            // both correction products over both dim halves first, the hi * hi product last
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                z0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl[0][dh], qh[b][dh], z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl[1][dh], qh[b][dh], z1, 0, 0, 0);
            }
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                z0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[0][dh], ql[b][dh], z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[1][dh], ql[b][dh], z1, 0, 0, 0);
            }
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                z0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[0][dh], qh[b][dh], z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[1][dh], qh[b][dh], z1, 0, 0, 0);
            }
            // lane (fr, fq): z0[r] = S[query fr][key kb*32 + fq*4 + r], z1[r] = same + 16
            if (EDGE) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (kb * 32 + fq * 4 + r >= len) z0[r] = -INFINITY;
                    if (kb * 32 + 16 + fq * 4 + r >= len) z1[r] = -INFINITY;
                }
            }
            float mx = CE_MAX2(CE_MAX2(CE_MAX2(z0[0], z0[1]), CE_MAX2(z0[2], z0[3])), CE_MAX2(CE_MAX2(z1[0], z1[1]), CE_MAX2(z1[2], z1[3])));
            {                                                         // lane ^ 16, lane ^ 32: issued by hand, see ce_attention_kernel
                float cp = mx;
                asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(mx), "+v"(cp));
                mx = CE_MAX2(mx, cp);
                cp = mx;
                asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(mx), "+v"(cp));
                mx = CE_MAX2(mx, cp);
            }
            const float mnew = CE_MAX2(mrun[b], mx);                // finite: key 0 is always real
            const float alpha = __builtin_amdgcn_exp2f((mrun[b] - mnew) * cs);
            mrun[b] = mnew;
            const float off = -mnew * cs;
            float e[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                e[r] = __builtin_amdgcn_exp2f(fmaf(z0[r], cs, off));
                e[4 + r] = __builtin_amdgcn_exp2f(fmaf(z1[r], cs, off));
            }
            lsum[b] = lsum[b] * alpha + (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
#pragma unroll
            for (int dq = 0; dq < 4; ++dq)
#pragma unroll
                for (int r = 0; r < 4; ++r) cx[b][dq][r] *= alpha;
            float eh[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) eh[r] = ce_trunc10(e[r]);
            const u32x4 ph_u = {ce_pk(eh[0], eh[1]), ce_pk(eh[2], eh[3]), ce_pk(eh[4], eh[5]), ce_pk(eh[6], eh[7])};
            const u32x4 pl_u = {ce_pk(e[0] - eh[0], e[1] - eh[1]), ce_pk(e[2] - eh[2], e[3] - eh[3]),
                                ce_pk(e[4] - eh[4], e[5] - eh[5]), ce_pk(e[6] - eh[6], e[7] - eh[7])};
            const half8 ph = __builtin_bit_cast(half8, ph_u), pl = __builtin_bit_cast(half8, pl_u);
            // ctx^T[d][q] += V^T[d][key] P[q][key]: A = V fragment (row d of quarter dq), B = P (col q = fr)
#pragma unroll
            for (int dq = 0; dq < 4; ++dq) cx[b][dq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl[dq], ph, cx[b][dq], 0, 0, 0);
#pragma unroll
            for (int dq = 0; dq < 4; ++dq) cx[b][dq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[dq], pl, cx[b][dq], 0, 0, 0);
#pragma unroll
            for (int dq = 0; dq < 4; ++dq) cx[b][dq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[dq], ph, cx[b][dq], 0, 0, 0);
        }
    };
    // STREAM, per block: wait for this wave's own DMAs of block kb (counted: `ahead` = its DMAs of the blocks staged after kb, which
    // stay in flight - 2 per block, none for a tile it skipped), barrier (block kb is complete; every wave is done with block kb - 1;
    // lgkmcnt(0) retires this wave's zero stores and fragment reads), stage block kb + CE_A64_RING - 1 into the slot of block kb - 1.
    auto stream_step = [&](const int kb) {
        const int last = min(kb + CE_A64_RING - 2, nkb - 1);          // the last block staged so far
        const int ahead = 2 * (last - kb) - (s_skip_last && last == nkb - 1 && last > kb ? 2 : 0);
        if (ahead >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (ahead == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kb + CE_A64_RING - 1 < nkb) stream_stage(kb + CE_A64_RING - 1);
    };
    static_assert(CE_A64_RING == 4, "stream_step's vmcnt cases cover two blocks ahead of the wait");
    if (STREAM) {
        for (int kb = 0; kb + 1 < nkb; ++kb) {
            stream_step(kb);
            if (has_rows) key_block(kb, std::false_type{});
        }
        stream_step(nkb - 1);
        if (has_rows) key_block(nkb - 1, std::true_type{});
    } else {
        for (int kb = 0; kb + 1 < nkb; ++kb) key_block(kb, std::false_type{});
        key_block(nkb - 1, std::true_type{});
    }
#undef CE_MAX2
    if (STREAM && !has_rows) return;
    // lane (fr, fq): cx[dq][r] = ctx[query fr][d = dq*16 + fq*4 + r]; the row sum is spread over the 4 fq lanes
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        float l = lsum[b];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        if ((qb0 + b) * 16 >= Lp) break;
        half_t* o = ctx16 + (row0 + (qb0 + b) * 16 + fr) * (2 * hidden) + head * 128 + fq * 4;
#pragma unroll
        for (int dq = 0; dq < 4; ++dq)                                // d quarter dq sits in K group dq >> 1 of the head, at dims (dq & 1) * 16..
            store_split4(o + (dq >> 1) * 64 + (dq & 1) * 16, 32, cx[b][dq][0] * inv, cx[b][dq][1] * inv, cx[b][dq][2] * inv, cx[b][dq][3] * inv);
    }
}

template <bool MX>
__global__ __launch_bounds__(256) void ce_pool_classify_kernel(const half_t* __restrict__ x16, const float* __restrict__ wp,
                                                                const float* __restrict__ bp, const float* __restrict__ wc,
                                                                const float* __restrict__ bc, const int32_t* __restrict__ pair_off,
                                                                int hidden, float* __restrict__ logits) {
    __shared__ float xs[1024];
    __shared__ float part[4];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const half_t* x = MX ? x16 : x16 + (size_t)pair_off[pair] * 2 * hidden;     // [CLS] = the pair's first packed row (split layout)
    // pair_off == nullptr (MX only): x16 holds one row per pair (the compact [CLS] stream of the last layer)
    for (int i = tid; i < hidden; i += 256)
        xs[i] = MX ? mx_load_elem(reinterpret_cast<const char*>(x16), pair_off ? pair_off[pair] : pair, i, hidden >> 5)
                   : (float)x[SPLIT_IDX(i)] + (float)x[SPLIT_IDX(i) + 32];
    __syncthreads();
    float acc = 0.f;
    for (int n = tid; n < hidden; n += 256) {
        float s = bp[n];
        const float* w = wp + (size_t)n * hidden;
        for (int k = 0; k < hidden; ++k) s += w[k] * xs[k];
        acc += wc[n] * tanhf(s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) part[wv] = acc;
    __syncthreads();
    if (tid == 0) logits[pair] = part[0] + part[1] + part[2] + part[3] + bc[0];
}

// The same head for the compact [CLS] stream of the MX forward (one row per pair), 8 pairs per workgroup: the pooler matrix is read
// once per 8 pairs and TRANSPOSED (wpT[k][n]: consecutive threads read consecutive floats) - the per-pair kernel above walks 590 KB of
// weights per pair with one row per thread (0.64 ms per 7,680 pairs). fp32 sums in the same k order as the kernel above.
#define POOL_PB 8
__global__ __launch_bounds__(256) void mx_pool_classify_kernel(const char* __restrict__ xc8, const float* __restrict__ wpT,
                                                                const float* __restrict__ bp, const float* __restrict__ wc,
                                                                const float* __restrict__ bc, int P, int hidden, float* __restrict__ logits) {
    __shared__ float xs[POOL_PB][1024];
    __shared__ float part[POOL_PB][4];
    const int p0 = blockIdx.x * POOL_PB, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < POOL_PB * hidden; i += 256) {
        const int j = i / hidden, c = i % hidden;
        xs[j][c] = p0 + j < P ? mx_load_elem(xc8, p0 + j, c, hidden >> 5) : 0.f;
    }
    __syncthreads();
    float acc[POOL_PB];
#pragma unroll
    for (int j = 0; j < POOL_PB; ++j) acc[j] = 0.f;
    for (int n = tid; n < hidden; n += 256) {
        float sj[POOL_PB];
        const float b = bp[n];
#pragma unroll
        for (int j = 0; j < POOL_PB; ++j) sj[j] = b;
        for (int k = 0; k < hidden; ++k) {
            const float w = wpT[(size_t)k * hidden + n];
#pragma unroll
            for (int j = 0; j < POOL_PB; ++j) sj[j] += w * xs[j][k];
        }
        const float c = wc[n];
#pragma unroll
        for (int j = 0; j < POOL_PB; ++j) acc[j] += c * tanhf(sj[j]);
    }
#pragma unroll
    for (int j = 0; j < POOL_PB; ++j) {
        float a = acc[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) part[j][wv] = a;
    }
    __syncthreads();
    if (tid < POOL_PB && p0 + tid < P) logits[p0 + tid] = part[tid][0] + part[tid][1] + part[tid][2] + part[tid][3] + bc[0];
}

// Sentence embedding head (sentence-transformers' Pooling + Normalize): mean of the last hidden state over the pair's real tokens,
// or (pool_cls: pooling_mode_cls_token) the last hidden state of row 0 alone, with no pooler dense / tanh; optionally L2-normalised.
// One workgroup per sequence; float32 sums over the split-fp16 stream (hi + lo).
template <bool MX>
__global__ __launch_bounds__(256) void ce_meanpool_kernel(const half_t* __restrict__ x16, const int32_t* __restrict__ pair_off,
                                                           const int32_t* __restrict__ lens, int L, int hidden, int normalize, int pool_cls,
                                                           float* __restrict__ out) {
    __shared__ float part[4];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int len = pool_cls ? 1 : max(1, min(lens[pair], L));       // [CLS] pooling: the "mean" of the first row (x / 1.0f is exact)
    const half_t* x = x16 + (size_t)pair_off[pair] * 2 * hidden;
    float sq = 0.f;
    float v[4] = {0.f, 0.f, 0.f, 0.f};                               // hidden <= 1024: up to 4 features per thread
    for (int e = 0, c = tid; c < hidden; c += 256, ++e) {
        float s = 0.f;
        for (int t = 0; t < len; ++t) {
            if (MX) { s += mx_load_elem(reinterpret_cast<const char*>(x16), (int64_t)pair_off[pair] + t, c, hidden >> 5); continue; }
            const half_t* r = x + (size_t)t * 2 * hidden + SPLIT_IDX(c);
            s += (float)r[0] + (float)r[32];
        }
        v[e] = s / (float)len;
        sq += v[e] * v[e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if (lane == 0) part[wv] = sq;
    __syncthreads();
    const float nrm = sqrtf(part[0] + part[1] + part[2] + part[3]);
    const float sc = normalize ? 1.0f / fmaxf(nrm, 1e-12f) : 1.0f;  // torch.nn.functional.normalize: x / max(||x||, eps)
    for (int e = 0, c = tid; c < hidden; c += 256, ++e) out[(size_t)pair * hidden + c] = v[e] * sc;
}

__global__ void ce_f32_split_kernel(const float* __restrict__ in, half_t* __restrict__ out, int64_t n, int cols) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int64_t row = i / cols;
        const int c = (int)(i % cols);
        const half_t hi = (half_t)in[i];
        half_t* o = out + row * 2 * cols + SPLIT_IDX(c);   // split-row layout: [hi 32 | lo 32] per 32-element K group
        o[0] = hi;
        o[32] = (half_t)(in[i] - (float)hi);
    }
}

// ---- token-vector and lexical heads of the embedder (rag_embed_multi_*; the three-headed bge-m3, the ColBERT checkpoints). Both read
// the last hidden state in the split layout, one wave per row, float32 sums in a fixed order: a row's outputs depend on that row alone.
// The MX forward's last hidden state is first rewritten from its image into the split layout (hi = fp16(x), lo = fp16(x - hi)).
__global__ void m3_mx_to_split_kernel(const char* __restrict__ x8, const int32_t* __restrict__ m_packed, int hidden, half_t* __restrict__ x16) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)m_packed[0] * hidden) return;
    const int64_t row = i / hidden;
    const int c = (int)(i % hidden);
    const float v = mx_load_elem(x8, row, c, hidden >> 5);
    const half_t hi = (half_t)v;
    half_t* o = x16 + row * 2 * hidden + SPLIT_IDX(c);
    o[0] = hi;
    o[32] = (half_t)(v - (float)hi);
}

// row_off[p] = sum over the texts before p of (clamped length - 1): where text p's token vectors start in the packed output;
// row_off[P] = the call's true total. The lengths are clamped as ce_pack_scan_kernel clamps them.
__global__ __launch_bounds__(1024) void m3_row_off_kernel(const int32_t* __restrict__ lens, int P, int L_in, int64_t* __restrict__ row_off) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int per = (P + 1023) / 1024;
    const int b = min(P, tid * per), e = min(P, b + per);
    long long s = 0;
    for (int p = b; p < e; ++p) s += max(1, min(lens[p], L_in)) - 1;
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const long long v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long off = part[tid] - s;
    for (int p = b; p < e; ++p) {
        row_off[p] = off;
        off += max(1, min(lens[p], L_in)) - 1;
    }
    if (tid == 1023) row_off[P] = part[1023];
}

// lexical head: out[p][t] = relu(lex_w . x[t] + lex_b) for t < len, 0 for len <= t < L_in. One wave per (text, position).
__global__ __launch_bounds__(256) void m3_lexical_kernel(const half_t* __restrict__ x16, const int32_t* __restrict__ pair_off,
                                                          const int32_t* __restrict__ clen, int P, int L_in, int hidden,
                                                          const float* __restrict__ lex_w, float lex_b, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= (int64_t)P * L_in) return;
    const int p = (int)(idx / L_in), t = (int)(idx % L_in);
    if (t >= clen[p]) {
        if (lane == 0) out[idx] = 0.f;
        return;
    }
    const half_t* r = x16 + ((size_t)pair_off[p] + t) * 2 * hidden;
    float s = 0.f;
    for (int c = lane; c < hidden; c += 64) s += ((float)r[SPLIT_IDX(c)] + (float)r[SPLIT_IDX(c) + 32]) * lex_w[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[idx] = fmaxf(s + lex_b, 0.f);
}

// token head, after its GEMM (raw = tok_W . x + tok_b, fp32 [packed row][tok_pad]): row t >= 1 of a text is L2-normalised
// (x / max(|x|, 1e-12)) and written to packed output row row_off[text] + t - 1; row 0 ([CLS]), the pad rows behind a length that is
// no multiple of 16 and every row at or past `cap` are skipped. One wave per packed row, tok_dim <= 1024 = 16 values per lane.
__global__ __launch_bounds__(256) void m3_tok_scatter_kernel(const float* __restrict__ raw, int tok_pad, int tok_dim,
                                                              const int32_t* __restrict__ m_packed, const int32_t* __restrict__ row_pair,
                                                              const int32_t* __restrict__ pair_off, const int32_t* __restrict__ clen,
                                                              const int64_t* __restrict__ row_off, int64_t cap, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m_packed[0]) return;
    const int pr = row_pair[row];
    const int t = (int)row - pair_off[pr];
    if (t < 1 || t >= clen[pr]) return;
    const int64_t dst = row_off[pr] + t - 1;
    if (dst >= cap) return;
    float v[16];
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + i * 64;
        v[i] = c < tok_dim ? raw[(size_t)row * tok_pad + c] : 0.f;
        sq += v[i] * v[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    const float sc = 1.0f / fmaxf(sqrtf(sq), 1e-12f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + i * 64;
        if (c < tok_dim) out[(size_t)dst * tok_dim + c] = v[i] * sc;
    }
}

// ------------------------------------------------------------------------------------------------
// Host side (launch() and raise_lds() are common.h's).
// ------------------------------------------------------------------------------------------------
// allocates n elements and enqueues their zero fill on st, the stream the forward runs on (a synchronous hipMemset on the null
// stream is NOT ordered against a non-blocking stream: the first forward after a reallocation could otherwise start before its
// buffers were cleared)
template <class T>
static int alloc_zeroed(rag_ctx* h, dev_buf<T>& b, size_t n, hipStream_t st) {
    if (int rc = b.alloc(h, n)) return rc;
    HIP_TRY(h, hipMemsetAsync(b, 0, n * sizeof(T), st));
    return RAG_OK;
}

// Drops workspace w and starts one for P pairs of L tokens: rows padded to 256, the chunk buffers allocated. pairs / L stay 0
// (nothing fits) until the caller has added its planes.
template <class W>
static int ws_renew(rag_ctx* h, W& w, int P, int L, int out_width, hipStream_t st) {
    HIP_TRY(h, hipStreamSynchronize(st));
    w = W();
    const int64_t Mp = w.tokens = round_up((int64_t)P * L, 256);
    ce_chunk_bufs& c = w.io;
    int rc;
    if ((rc = c.ids.alloc(h, (size_t)Mp))) return rc;
    if ((rc = c.tt.alloc(h, (size_t)Mp))) return rc;
    if ((rc = c.lens.alloc(h, (size_t)P))) return rc;
    if ((rc = c.clen.alloc(h, (size_t)P))) return rc;
    if ((rc = c.pair_off.alloc(h, (size_t)P + 1))) return rc;
    if ((rc = c.row_off.alloc(h, (size_t)P + 1))) return rc;
    if ((rc = c.row_pair.alloc(h, (size_t)Mp))) return rc;
    if ((rc = c.row_att.alloc(h, (size_t)Mp))) return rc;
    if ((rc = c.m_packed.alloc(h, 1))) return rc;
    if ((rc = c.sid.alloc(h, (size_t)P * L))) return rc;              // L_in <= L
    if ((rc = c.stt.alloc(h, (size_t)P * L))) return rc;
    return c.logits.alloc(h, (size_t)P * out_width);
}

void ce_free(rag_ctx* h) {
    delete h->ce;
    delete h->emb;
    h->ce = h->emb = nullptr;
}

static int up_f32(rag_ctx* h, const float* src, size_t n, dev_buf<float>& dst) {
    if (int rc = dst.alloc(h, n)) return rc;
    HIP_TRY(h, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    return RAG_OK;
}

// rows of several fp32 host matrices (same `cols`) concatenated -> one device matrix in both operand formats: split fp16 (hi
// plane | lo plane) in dst16 and, when the MX forward can run the model (mx), the hi16 + lo8 image tensor (ce_mx.h) in dst8
static int up_weight(rag_ctx* h, std::vector<const float*> srcs, size_t rows_each, size_t cols, dev_buf<half_t>& dst16,
                     dev_buf<char>& dst8, bool mx) {
    const size_t n_each = rows_each * cols, total = n_each * srcs.size();
    const dim3 grid((unsigned)((total + 255) / 256));
    dev_buf<float> tmp;
    int rc;
    if ((rc = tmp.alloc(h, total))) return rc;
    for (size_t i = 0; i < srcs.size(); ++i)
        HIP_TRY(h, hipMemcpyAsync(tmp + i * n_each, srcs[i], n_each * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if ((rc = dst16.alloc(h, 2 * total))) return rc;
    launch(ce_f32_split_kernel, grid, dim3(256), 0, h->stream, tmp, dst16, (int64_t)total, (int)cols);
    if (mx) {
        if ((rc = dst8.alloc(h, 3 * total))) return rc;
        launch(mx_pack_weight_kernel, grid, dim3(256), 0, h->stream, tmp, (int)(rows_each * srcs.size()), (int)cols, dst8);
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));              // tmp is freed on return
    return RAG_OK;
}

// Tensor order (HF state-dict names), see optimized-rag_amd/cross_encoder.py::flatten_state_dict:
//  0 word, 1 position, 2 token_type, 3 emb LN weight, 4 emb LN bias,
//  per layer (16): q.w q.b k.w k.b v.w v.b attn.out.w attn.out.b attn.LN.w attn.LN.b inter.w inter.b out.w out.b out.LN.w out.LN.b
//  then pooler.w pooler.b classifier.w classifier.b
//  (an embedding model - BertModel behind a mean-pooling head - ends after the layers: no pooler / classifier tensors)
static int ce_probe_mx(rag_ctx* h, rag_ce_model* m);
// Head dim: 32 at every hidden size, 64 at every hidden size the split-fp16 forward alone serves (128, 256, 512, 640, 768, 896, 1024).
// Hidden 384 belongs to the MX forward, whose operand images and attention instances are laid out per 32-wide head: it keeps 32 only.
static int ce_load_model(rag_ctx* h, const rag_ce_config* cfg, const float* const* T, int n, bool embed, int flags, rag_ce_model** slot) {
    ARG_CHECK(h, cfg && T, "ce_load: null");
    ARG_CHECK(h, cfg->hidden % 128 == 0 && cfg->hidden <= 1024 && cfg->ffn % 128 == 0, "ce_load: hidden/ffn must be multiples of 128");
    ARG_CHECK(h, cfg->heads > 0 && cfg->hidden % cfg->heads == 0, "ce_load: hidden must be a multiple of heads");
    const int d_head = cfg->hidden / cfg->heads;
    ARG_CHECK(h, d_head == 32 || d_head == 64, "ce_load: head dim must be 32 or 64");
    ARG_CHECK(h, d_head == 32 || cfg->hidden != MX_TM, "ce_load: hidden 384 (the MX forward's width) takes head dim 32 only");
    ARG_CHECK(h, (flags & ~(RAG_EMBED_NORMALIZE | RAG_EMBED_POOL_CLS)) == 0, "embed_load: unknown flag bits");
    ARG_CHECK(h, n == 5 + 16 * cfg->layers + (embed ? 0 : 4), "ce_load: wrong tensor count");
    delete *slot;
    rag_ce_model* m = *slot = new rag_ce_model();
    m->cfg = *cfg;
    m->embed = embed;
    m->normalize = (flags & RAG_EMBED_NORMALIZE) != 0;
    m->pool_cls = (flags & RAG_EMBED_POOL_CLS) != 0;
    m->d_head = d_head;
    m->out_width = embed ? cfg->hidden : 1;
    const size_t H = cfg->hidden, F = cfg->ffn;
    int rc;
    if ((rc = up_f32(h, T[0], (size_t)cfg->vocab_size * H, m->word))) return rc;
    if ((rc = up_f32(h, T[1], (size_t)cfg->max_pos * H, m->pos))) return rc;
    if (cfg->type_vocab == 1) {
        // one token type (RoBERTa / XLM-R): the forward indexes the table with `token_type != 0`, so the row is uploaded twice -
        // every token takes row 0's values whatever token_type_ids holds
        if ((rc = m->type.alloc(h, 2 * H))) return rc;
        HIP_TRY(h, hipMemcpyAsync(m->type, T[2], H * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(m->type + H, T[2], H * sizeof(float), hipMemcpyHostToDevice, h->stream));
    } else if ((rc = up_f32(h, T[2], (size_t)cfg->type_vocab * H, m->type))) return rc;
    if ((rc = up_f32(h, T[3], H, m->emb_ln_g))) return rc;
    if ((rc = up_f32(h, T[4], H, m->emb_ln_b))) return rc;
    m->layers.resize(cfg->layers);
    const bool mx = m->mx_ok = H == MX_TM && F % MX_TM == 0 && F <= 1536;    // one feature tile = the hidden state (LayerNorm in the epilogue); the FFN bias is staged in 6 KiB of LDS
    for (int l = 0; l < cfg->layers; ++l) {
        const float* const* t = T + 5 + 16 * l;
        auto& ly = m->layers[l];
        if ((rc = up_weight(h, {t[0], t[2], t[4]}, H, H, ly.wqkv, ly.wqkv8, mx))) return rc;
        std::vector<float> bq(3 * H);
        std::memcpy(bq.data(), t[1], H * 4); std::memcpy(bq.data() + H, t[3], H * 4); std::memcpy(bq.data() + 2 * H, t[5], H * 4);
        if ((rc = up_f32(h, bq.data(), 3 * H, ly.bqkv))) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));          // bq is a stack-lifetime buffer
        if ((rc = up_weight(h, {t[6]}, H, H, ly.wo, ly.wo8, mx))) return rc;
        if ((rc = up_f32(h, t[7], H, ly.bo))) return rc;
        if ((rc = up_f32(h, t[8], H, ly.ln1_g))) return rc;
        if ((rc = up_f32(h, t[9], H, ly.ln1_b))) return rc;
        if ((rc = up_weight(h, {t[10]}, F, H, ly.w1, ly.w18, mx))) return rc;
        if ((rc = up_f32(h, t[11], F, ly.b1))) return rc;
        if ((rc = up_weight(h, {t[12]}, H, F, ly.w2, ly.w28, mx))) return rc;
        if ((rc = up_f32(h, t[13], H, ly.b2))) return rc;
        if ((rc = up_f32(h, t[14], H, ly.ln2_g))) return rc;
        if ((rc = up_f32(h, t[15], H, ly.ln2_b))) return rc;
    }
    if (!embed) {
        const float* const* t = T + 5 + 16 * cfg->layers;
        if ((rc = up_f32(h, t[0], H * H, m->wp))) return rc;
        {
            std::vector<float> tr(H * H);
            for (size_t n = 0; n < H; ++n)
                for (size_t k = 0; k < H; ++k) tr[k * H + n] = t[0][n * H + k];
            if ((rc = up_f32(h, tr.data(), H * H, m->wpT))) return rc;
            HIP_TRY(h, hipStreamSynchronize(h->stream));          // tr is a stack-lifetime buffer
        }
        if ((rc = up_f32(h, t[1], H, m->bp))) return rc;
        if ((rc = up_f32(h, t[2], H, m->wc))) return rc;
        if ((rc = up_f32(h, t[3], 1, m->bc))) return rc;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return m->mx_ok && !embed ? ce_probe_mx(h, m) : RAG_OK;
}

int ce_load_host(rag_ctx* h, const rag_ce_config* cfg, const float* const* T, int n) {
    return ce_load_model(h, cfg, T, n, false, 0, &h->ce);
}

int embed_load_host(rag_ctx* h, const rag_ce_config* cfg, const float* const* T, int n, int flags) {
    return ce_load_model(h, cfg, T, n, true, flags, &h->emb);
}

// The attention length classes a call's seq_len is rounded up to. Up to 512: both head widths and both forwards. Above: models with
// 64-wide heads alone (ce_attention_kernel keeps a pair's K / V in LDS, the MX forward is laid out per 32-wide head, and no
// long-context checkpoint has 32-wide heads).
static const int kAttnL[] = {32, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192};
static int ce_width_limit(int d_head) { return d_head == 64 ? 8192 : 512; }
// the class of seq_len for a head width, 0 when there is none (host only)
int ce_length_class(int d_head, int seq_len) {
    if ((d_head != 32 && d_head != 64) || seq_len < 1 || seq_len > ce_width_limit(d_head)) return 0;
    for (int c : kAttnL) if (c >= seq_len) return c;
    return 0;
}
// the longest seq_len a call on model m may have: the position table or the head width's limit, whichever is smaller
static int ce_seq_limit(const rag_ce_model* m) { return std::min(m->cfg.max_pos, ce_width_limit(m->d_head)); }
int ce_model_seq_limit(const rag_ctx* h, int which) {
    const rag_ce_model* m = which == 0 ? h->ce : h->emb;
    return m ? ce_seq_limit(m) : 0;
}

// halfs per K / V fragment plane of Mp padded rows (both forwards)
static size_t kv_plane_halfs(int64_t Mp, size_t H) { return (size_t)Mp * H + 2048; }
// persistent GEMM grid: one workgroup per compute unit, a multiple of 8 (the XCD-aware tile map)
static unsigned ce_gemm_grid(const rag_ctx* h) { return (unsigned)(h->n_cu >= 8 ? h->n_cu / 8 * 8 : 256); }

// One chunk of a call, all device pointers: [P][L_in] token / type ids, the P lengths as the caller gave them and the chunk's
// [P][out_width] result slots (the workspace's staging buffers for host-pointer calls, the caller's own arrays otherwise); L is
// the attention length class L_in was rounded up to.
struct ce_chunk {
    const int32_t *ids, *tt, *lens;
    float* out;
    int P, L_in, L;
    // rag_embed_multi_* alone (then `out` may be null: no pooled vector asked for): the chunk's [P][L_in] lexical weights, the
    // call's packed token vectors with the chunk's slice of the row offsets, each null when not asked for
    float* lex = nullptr;
    float* tok = nullptr;
    const int64_t* row_off = nullptr;
    int64_t tok_cap = 0;
};

// pads [P][L_in] token arrays to the supported attention length L (>= L_in), pad id 0 / type 0
__global__ void ce_pad_tokens_kernel(const int32_t* __restrict__ in_ids, const int32_t* __restrict__ in_tt, int P, int L_in, int L,
                                     int32_t* __restrict__ ids, int32_t* __restrict__ tt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)P * L) return;
    const int p = (int)(i / L), t = (int)(i % L);
    ids[i] = t < L_in ? in_ids[(size_t)p * L_in + t] : 0;
    tt[i] = t < L_in ? in_tt[(size_t)p * L_in + t] : 0;
}

// Start of every chunk: tokens padded to L, then the packed row layout (no host round trip: grids cover the padded worst case,
// kernels stop at m_packed). Every later kernel reads the clamped lengths the scan writes (io.clen), never c.lens.
// g = granularity of the GEMM row space (4 or 16; 16: io.row_off = io.pair_off, one row space)
static void chunk_prologue(const ce_ws_base& w, const ce_chunk& c, int g, hipStream_t st) {
    const ce_chunk_bufs& io = w.io;
    launch(ce_pad_tokens_kernel, dim3((unsigned)(((int64_t)c.P * c.L + 255) / 256)), dim3(256), 0, st, c.ids, c.tt, c.P, c.L_in, c.L, io.ids, io.tt);
    launch(ce_pack_scan_kernel, dim3(1), dim3(1024), 0, st, c.lens, c.P, c.L_in, g, io.clen, io.pair_off, io.row_off, io.m_packed);
    launch(ce_pack_rows_kernel, dim3((unsigned)((w.tokens + 255) / 256)), dim3(256), 0, st, io.pair_off, io.row_off, c.P, c.L, w.tokens, io.row_pair,
           io.row_att);
}

// Attention of one layer: one workgroup per (head, pair), QB 16-query blocks per wave, on the forward's Q / K / V planes into
// ctx (MX: the image tensor, which the kernel writes as bytes). max_qblocks = 1 (MX only) is the [CLS]-only last layer of a
// classifier: one wave per (head, pair), no LDS.
template <int QB, bool MX>
static int launch_attention(rag_ctx* h, const rag_ce_model* m, const ce_ws_base& w, const half_t* q, const half_t* kf, const half_t* vf,
                            half_t* ctx, const ce_chunk& c, hipStream_t st, int max_qblocks = 1 << 20) {
    const int H = m->cfg.hidden, heads = m->cfg.heads, L = c.L;
    const size_t kv_plane = kv_plane_halfs(w.tokens, H);
    const dim3 grid(heads, c.P);
    if constexpr (MX)
        if (max_qblocks == 1) {
            launch(ce_attention_kernel<1, true, true>, grid, dim3(64), 0, st, q, kf, vf, kv_plane, w.io.clen, w.io.pair_off, w.io.row_off, L, H,
                   heads, (int)w.tokens, ctx, 1);
            return RAG_OK;
        }
    const int lds = L * 256;                                           // K hi | K lo | V hi | V lo fragment planes
    if (int rc = raise_lds(h, h->attr_ce_attn_lds[MX][QB], lds, ce_attention_kernel<QB, MX>)) return rc;
    launch(ce_attention_kernel<QB, MX>, grid, dim3(64 * (L / (16 * QB))), lds, st, q, kf, vf, kv_plane, w.io.clen, w.io.pair_off, w.io.row_off, L,
           H, heads, (int)w.tokens, ctx, max_qblocks);
    return RAG_OK;
}

// Attention of one layer of a model with 64-wide heads (split-fp16 forward): two 16-query blocks per wave in every length class. Up
// to class 256 the (head, pair)'s four K / V planes are staged in LDS (512 B per key, 128 KiB at 256); classes 384 and 512 would
// need 192 and 256 KiB, so they read the fragments from global memory, take no LDS, and run as two workgroups of 8 waves per
// (head, pair). The classes above 512 run L / 256 such workgroups per (head, pair): the streamed form (a 64-KiB LDS ring shared by
// the workgroup's waves) from CE_A64_STREAM_FROM on, DIRECT below it: measured at 768, 1024, 1536, 2048, 4096 and 8192, the
// streamed form is the faster one at every class by more than the round-to-round spread (0.9 % of an embedding forward at 768,
// 6.1 % at 8192; profiles/ce_long_seq.json); 384 and 512 were neither measured nor switched. Option ce_attn_stream (a diagnostic: the two forms return
// the same bits and can be timed against each other, tools/ce_long_time.py): -1 = DIRECT at every class above 256, 1 = streamed
// at every class above 512 whatever the default there, 0 = the default.
#define CE_A64_STREAM_FROM 768
static int launch_attention64(rag_ctx* h, const rag_ce_model* m, const ce_split_ws& w, const ce_chunk& c, hipStream_t st) {
    const int H = m->cfg.hidden, L = c.L;
    const size_t kv_plane = kv_plane_halfs(w.tokens, H);
    const dim3 grid(m->cfg.heads, c.P), block(64 * (L / 32));
    const dim3 zgrid(m->cfg.heads, c.P, (L + 255) / 256);             // workgroups of 256 queries
    if (L <= 256) {
        const int lds = L * 512;                                       // K hi | K lo | V hi | V lo fragment planes
        if (int rc = raise_lds(h, h->attr_ce_attn64_lds, lds, ce_attention64_kernel<CE_A64_RESIDENT>)) return rc;
        launch(ce_attention64_kernel<CE_A64_RESIDENT>, grid, block, lds, st, w.q16, w.kf16, w.vf16, kv_plane, w.io.clen, w.io.pair_off, L, H,
               (int)w.tokens, w.ctx16);
    } else if (L > 512 && h->opt.ce_attn_stream >= 0 && (L >= CE_A64_STREAM_FROM || h->opt.ce_attn_stream > 0)) {
        const int lds = CE_A64_RING * CE_A64_SLOT;
        if (int rc = raise_lds(h, h->attr_ce_attn64s_lds, lds, ce_attention64_kernel<CE_A64_STREAM>)) return rc;
        launch(ce_attention64_kernel<CE_A64_STREAM>, zgrid, dim3(512), lds, st, w.q16, w.kf16, w.vf16, kv_plane, w.io.clen, w.io.pair_off, L, H,
               (int)w.tokens, w.ctx16);
    } else
        launch(ce_attention64_kernel<CE_A64_DIRECT>, zgrid, dim3(512), 0, st, w.q16, w.kf16, w.vf16, kv_plane, w.io.clen, w.io.pair_off, L, H,
               (int)w.tokens, w.ctx16);
    return RAG_OK;
}

// ---- the split-fp16 forward ------------------------------------------------------------------------------------------
static int ce_ensure_ws(rag_ctx* h, rag_ce_model* m, int P, int L, hipStream_t st) {
    ce_split_ws& w = m->split;
    if (w.fits(P, L)) return RAG_OK;
    int rc;
    if ((rc = ws_renew(h, w, P, L, m->out_width, st))) return rc;
    const size_t H = m->cfg.hidden, F = m->cfg.ffn, rows = (size_t)w.tokens, kv = kv_plane_halfs(w.tokens, H);
    // padded token rows are read by the GEMM tiles: keep them finite
    if ((rc = alloc_zeroed(h, w.x16, 2 * rows * H, st))) return rc;
    if ((rc = alloc_zeroed(h, w.q16, 2 * rows * H, st))) return rc;
    if ((rc = alloc_zeroed(h, w.kf16, 2 * kv, st))) return rc;
    if ((rc = alloc_zeroed(h, w.vf16, 2 * kv, st))) return rc;
    if ((rc = alloc_zeroed(h, w.ctx16, 2 * rows * H, st))) return rc;
    if ((rc = alloc_zeroed(h, w.h16, 2 * rows * F, st))) return rc;
    if ((rc = alloc_zeroed(h, w.y32, rows * H, st))) return rc;
    w.pairs = P;
    w.L = L;
    return RAG_OK;
}

// calls f(std::integral_constant<int, hidden / 64>()): the per-lane feature count the embedding and LayerNorm kernels are built for
template <class F>
static int per_lane_dispatch(rag_ctx* h, int hidden, F&& f) {
    switch (hidden / 64) {
        case 2: f(std::integral_constant<int, 2>()); break; case 4: f(std::integral_constant<int, 4>()); break; case 6: f(std::integral_constant<int, 6>()); break;
        case 8: f(std::integral_constant<int, 8>()); break; case 10: f(std::integral_constant<int, 10>()); break; case 12: f(std::integral_constant<int, 12>()); break;
        case 14: f(std::integral_constant<int, 14>()); break; case 16: f(std::integral_constant<int, 16>()); break;
        default: h->err = "ce: unsupported hidden size"; return RAG_ERR_ARG;
    }
    return RAG_OK;
}

// LayerNorm of the residual sums y32 -> x16, one wave per token
static int ce_layernorm(rag_ctx* h, const rag_ce_model* m, const float* g, const float* b, int64_t M, hipStream_t st) {
    const ce_split_ws& w = m->split;
    return per_lane_dispatch(h, m->cfg.hidden, [&](auto per) {
        launch(ce_layernorm_kernel<decltype(per)::value>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, w.y32, g, b, w.io.m_packed,
               m->cfg.hidden, (float)m->cfg.ln_eps, w.x16);
    });
}

// one split-fp16 GEMM over all packed rows: N output features over K, epilogue E; the outputs an epilogue does not write are null
template <int E>
static void ce_gemm(rag_ctx* h, const rag_ce_model* m, hipStream_t st, const half_t* W, const half_t* X, int N, int K, const float* bias,
                    const half_t* resid, float* out32, half_t* out16, half_t* kf = nullptr, half_t* vf = nullptr, size_t kv_plane = 0) {
    const ce_split_ws& w = m->split;
    launch(ce_gemm_kernel<E>, dim3(ce_gemm_grid(h)), dim3(512), CE_GEMM_LDS, st, W, X, N, K, bias, resid, out32, out16, kf, vf, kv_plane,
           m->cfg.hidden, m->cfg.heads, w.io.m_packed, (int)w.tokens);
}

// The heads of one chunk on its last hidden state x16 (split layout; w = the workspace of the forward that ran). Lexical: one dot
// per (text, position). Token vectors: the split-fp16 GEMM with the fp32 epilogue over all packed rows, then normalise + scatter.
static int heads_chunk(rag_ctx* h, rag_ce_model* m, const ce_ws_base& w, const half_t* x16, const ce_chunk& c, hipStream_t st) {
    ce_heads& hd = m->heads;
    const ce_chunk_bufs& io = w.io;
    const int H = m->cfg.hidden;
    if (c.lex)
        launch(m3_lexical_kernel, dim3((unsigned)(((int64_t)c.P * c.L_in + 3) / 4)), dim3(256), 0, st, x16, io.pair_off, io.clen, c.P, c.L_in, H,
               hd.lex_w, hd.lex_b, c.lex);
    if (c.tok) {
        if (int rc = raise_lds(h, h->attr_m3_gemm_lds, CE_GEMM_LDS, ce_gemm_kernel<EPI_F32>)) return rc;
        launch(ce_gemm_kernel<EPI_F32>, dim3(ce_gemm_grid(h)), dim3(512), CE_GEMM_LDS, st, hd.tok_w, x16, hd.tok_pad, H, hd.tok_b, nullptr, hd.raw,
               nullptr, nullptr, nullptr, (size_t)0, H, m->cfg.heads, io.m_packed, (int)w.tokens);
        launch(m3_tok_scatter_kernel, dim3((unsigned)(((int64_t)c.P * c.L + 3) / 4)), dim3(256), 0, st, hd.raw, hd.tok_pad, hd.tok_dim, io.m_packed,
               io.row_pair, io.pair_off, io.clen, c.row_off, c.tok_cap, c.tok);
    }
    return RAG_OK;
}

static int ce_forward_chunk(rag_ctx* h, rag_ce_model* m, const ce_chunk& c, hipStream_t st) {
    ce_split_ws& w = m->split;                                         // plane strides follow the ALLOCATED size (w.tokens)
    const ce_chunk_bufs& io = w.io;
    const int H = m->cfg.hidden, F = m->cfg.ffn, P = c.P, L = c.L;
    const int64_t M = (int64_t)P * L;
    int rc;
    if ((rc = raise_lds(h, h->attr_ce_gemm_lds, CE_GEMM_LDS, ce_gemm_kernel<EPI_QKV>, ce_gemm_kernel<EPI_GELU>, ce_gemm_kernel<EPI_RESID>,
                        ce_gemm_kernel<EPI_QKV64>)))
        return rc;
    chunk_prologue(w, c, 16, st);
    rc = per_lane_dispatch(h, H, [&](auto per) {
        launch(ce_embed_ln_kernel<decltype(per)::value>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, io.ids, io.tt, m->word, m->pos,
               m->type, m->emb_ln_g, m->emb_ln_b, io.m_packed, io.row_pair, io.pair_off, L, H, m->cfg.vocab_size, m->cfg.max_pos, (float)m->cfg.ln_eps, w.x16);
    });
    if (rc) return rc;
    for (const auto& ly : m->layers) {
        if (m->d_head == 64) {
            ce_gemm<EPI_QKV64>(h, m, st, ly.wqkv, w.x16, 3 * H, H, ly.bqkv, nullptr, nullptr, w.q16, w.kf16, w.vf16, kv_plane_halfs(w.tokens, H));
            rc = launch_attention64(h, m, w, c, st);
        } else {
            ce_gemm<EPI_QKV>(h, m, st, ly.wqkv, w.x16, 3 * H, H, ly.bqkv, nullptr, nullptr, w.q16, w.kf16, w.vf16, kv_plane_halfs(w.tokens, H));
            rc = L == 32 ? launch_attention<1, false>(h, m, w, w.q16, w.kf16, w.vf16, w.ctx16, c, st)
                         : launch_attention<2, false>(h, m, w, w.q16, w.kf16, w.vf16, w.ctx16, c, st);
        }
        if (rc) return rc;
        // out-projection + bias + residual -> y32, then LayerNorm -> x16
        ce_gemm<EPI_RESID>(h, m, st, ly.wo, w.ctx16, H, H, ly.bo, w.x16, w.y32, nullptr);
        if ((rc = ce_layernorm(h, m, ly.ln1_g, ly.ln1_b, M, st))) return rc;
        // FFN: up-projection + bias + GELU -> h16, down-projection + bias + residual -> y32, then LayerNorm -> x16
        ce_gemm<EPI_GELU>(h, m, st, ly.w1, w.x16, F, H, ly.b1, nullptr, nullptr, w.h16);
        ce_gemm<EPI_RESID>(h, m, st, ly.w2, w.h16, H, F, ly.b2, w.x16, w.y32, nullptr);
        if ((rc = ce_layernorm(h, m, ly.ln2_g, ly.ln2_b, M, st))) return rc;
    }
    if (m->embed) {
        if (c.out) launch(ce_meanpool_kernel<false>, dim3(P), dim3(256), 0, st, w.x16, io.pair_off, io.clen, L, H, m->normalize, m->pool_cls, c.out);
        if (c.lex || c.tok)
            if ((rc = heads_chunk(h, m, w, w.x16, c, st))) return rc;
    } else
        launch(ce_pool_classify_kernel<false>, dim3(P), dim3(256), 0, st, w.x16, m->wp, m->bp, m->wc, m->bc, io.pair_off, H, c.out);
    HIP_TRY(h, hipGetLastError());
    return RAG_OK;
}

// ---- the MX forward (ce_mx.h): every GEMM on 384-feature x 128-token tiles with hi16 + lo8 operands ---------------------
// The FFN of a layer tail as one launch (mx_ffn_kernel) or as two (FFN-up -> h8 -> FFN-down). Option ce_ffn_fused: 1 = one launch,
// -1 = two, 0 = one wherever every workgroup's slot of the intermediate fits the 256 MiB Infinity Cache together with the operands
// streaming past it: at most 192 MiB of slots. (256 workgroups at ffn 1536 are 144 MiB, so every shape the MX forward takes today
// is under the cap; it is there for a wider grid or ffn.) Either way the same bits: the choice is one of speed and workspace.
#define MX_FFN_SLOT_CAP ((size_t)192 << 20)
static size_t mx_ffn_slots_bytes(const rag_ctx* h, const rag_ce_model* m) { return (size_t)ce_gemm_grid(h) * mx_ffn_slot_bytes(m->cfg.ffn); }
static bool mx_ffn_fused(const rag_ctx* h, const rag_ce_model* m) {
    return h->opt.ce_ffn_fused > 0 || (h->opt.ce_ffn_fused == 0 && mx_ffn_slots_bytes(h, m) <= MX_FFN_SLOT_CAP);
}

// The intermediate of the FFN form in force (option ce_ffn_fused): the slots, or h8 / hc8. Only that form's buffers are allocated,
// the other's when the option is first switched on this workspace.
static int mx_ensure_ffn(rag_ctx* h, rag_ce_model* m, hipStream_t st) {
    ce_mx_ws& w = m->mx;
    int rc;
    if (mx_ffn_fused(h, m)) return w.ffn_slots ? RAG_OK : alloc_zeroed(h, w.ffn_slots, mx_ffn_slots_bytes(h, m), st);
    if (w.h8) return RAG_OK;
    const size_t F = m->cfg.ffn;
    if ((rc = alloc_zeroed(h, w.h8, (size_t)w.tokens * F * 3, st))) return rc;
    return alloc_zeroed(h, w.hc8, (size_t)round_up((int64_t)w.pairs, MX_TN) * F * 3, st);
}

static int mx_ensure_ws(rag_ctx* h, rag_ce_model* m, int P, int L, hipStream_t st) {
    ce_mx_ws& w = m->mx;
    if (w.fits(P, L)) return mx_ensure_ffn(h, m, st);
    int rc;
    if ((rc = ws_renew(h, w, P, L, m->out_width, st))) return rc;
    const size_t H = m->cfg.hidden, rows = (size_t)w.tokens, kv = kv_plane_halfs(w.tokens, H);
    const size_t cls_rows = (size_t)round_up((int64_t)P, MX_TN);
    // rows past a chunk's packed rows are read by the last token tile of every GEMM: keep them finite (zero is a valid image)
    if ((rc = alloc_zeroed(h, w.x8, rows * H * 3, st))) return rc;
    if ((rc = alloc_zeroed(h, w.ctx8, rows * H * 3, st))) return rc;
    if ((rc = alloc_zeroed(h, w.xc8, cls_rows * H * 3, st))) return rc;
    if ((rc = alloc_zeroed(h, w.cc8, cls_rows * H * 3, st))) return rc;
    if ((rc = w.m_cls.alloc(h, 1))) return rc;                         // written by every gather before it is read
    if ((rc = alloc_zeroed(h, w.qf16, 2 * kv, st))) return rc;
    if ((rc = alloc_zeroed(h, w.kf16, 2 * kv, st))) return rc;
    if ((rc = alloc_zeroed(h, w.vf16, 2 * kv, st))) return rc;
    w.pairs = P;
    w.L = L;
    return mx_ensure_ffn(h, m, st);
}

// one MX GEMM over `rows[0]` token rows of X: nk K-steps, n_ft feature tiles of W, epilogue epi
template <class EPI>
static void mx_gemm(rag_ctx* h, hipStream_t st, const char* W, const char* X, int nk, int n_ft, const int32_t* rows, EPI epi) {
    launch(mx_gemm_kernel<EPI>, dim3(ce_gemm_grid(h)), dim3(512), MX_KERNEL_LDS, st, W, X, nk, n_ft, rows, epi);
}

// QKV projection of the rows[0] rows of X: n_ft feature tiles of (Q, K, V) from tile ft_base on. row_map / n_map: Q of compact
// rows is scattered to the token rows row_map names (mx_epi_qkv).
static void mx_qkv(rag_ctx* h, const rag_ce_model* m, const rag_ce_model::Layer& ly, hipStream_t st, int ft_base, int n_ft, const char* X,
                   const int32_t* rows, const int32_t* row_map = nullptr, int n_map = 0) {
    const ce_mx_ws& w = m->mx;
    const int nk = m->cfg.hidden / 32;
    mx_gemm(h, st, ly.wqkv8 + (size_t)ft_base * nk * MX_A_STAGE, X, nk, n_ft, rows,
            mx_epi_qkv{w.qf16, w.kf16, w.vf16, kv_plane_halfs(w.tokens, m->cfg.hidden), ly.bqkv, (int)(w.tokens >> 4), ft_base, w.io.row_att,
                       row_map, n_map});
}

// The layer after its attention, on rows[0] rows: out-projection + bias + residual + LayerNorm (attn -> x, in place), FFN-up +
// bias + GELU (x -> ffn), FFN-down + bias + residual + LayerNorm (ffn -> x, in place). The two FFN GEMMs are one launch over the
// workspace's slots (mx_ffn_kernel; `ffn` is then not touched) or two launches through `ffn` (mx_ffn_fused).
static void mx_layer_tail(rag_ctx* h, const rag_ce_model* m, const rag_ce_model::Layer& ly, hipStream_t st, const char* attn, char* x,
                          char* ffn, const int32_t* rows) {
    const int H = m->cfg.hidden, F = m->cfg.ffn;
    const float eps = (float)m->cfg.ln_eps;
    mx_gemm(h, st, ly.wo8, attn, H / 32, 1, rows, mx_epi_ln{x, ly.bo, ly.ln1_g, ly.ln1_b, eps});
    if (mx_ffn_fused(h, m)) {
        launch(mx_ffn_kernel, dim3(ce_gemm_grid(h)), dim3(512), MX_FFN_LDS, st, ly.w18, ly.w28, F / MX_TM, rows,
               mx_epi_gelu{m->mx.ffn_slots, ly.b1, F / 32}, mx_epi_ln{x, ly.b2, ly.ln2_g, ly.ln2_b, eps});
        return;
    }
    mx_gemm(h, st, ly.w18, x, H / 32, F / MX_TM, rows, mx_epi_gelu{ffn, ly.b1, F / 32});
    mx_gemm(h, st, ly.w28, ffn, F / 32, 1, rows, mx_epi_ln{x, ly.b2, ly.ln2_g, ly.ln2_b, eps});
}

static int mx_forward_chunk(rag_ctx* h, rag_ce_model* m, const ce_chunk& c, hipStream_t st) {
    ce_mx_ws& w = m->mx;
    const ce_chunk_bufs& io = w.io;
    const int H = m->cfg.hidden, P = c.P, L = c.L;
    int rc;
    if ((rc = raise_lds(h, h->attr_ce_mx_lds, MX_KERNEL_LDS, mx_gemm_kernel<mx_epi_qkv>, mx_gemm_kernel<mx_epi_gelu>, mx_gemm_kernel<mx_epi_ln>)))
        return rc;
    if ((rc = raise_lds(h, h->attr_ce_ffn_lds, MX_FFN_LDS, mx_ffn_kernel))) return rc;
    // A classifier packs its GEMM rows in fours: only attention needs a pair on whole 16-row tiles (its Q / K / V fragments), the GEMMs
    // work on 128-row image tiles wherever a pair starts, and the V epilogue stores four consecutive keys per lane. Every GEMM,
    // LayerNorm, GELU and embedding row between a length rounded up to 4 and to 16 is work no result needs. An embedding model keeps
    // 16: its pooling and token heads read rows through pair_off.
    chunk_prologue(w, c, m->embed ? 16 : 4, st);
    launch(mx_embed_ln_kernel, dim3((unsigned)(((int64_t)P * L + MX_EMB_ROWS - 1) / MX_EMB_ROWS)), dim3(256), 0, st, io.ids, io.tt, m->word,
           m->pos, m->type, m->emb_ln_g, m->emb_ln_b, io.m_packed, io.row_pair, io.row_off, L, m->cfg.vocab_size, (float)m->cfg.ln_eps, w.x8);
    half_t* const ctx = reinterpret_cast<half_t*>(w.ctx8.get());       // the attention kernel writes the image tensor as bytes
    const dim3 gather_grid((unsigned)(((int64_t)P * 72 + 255) / 256));
    // The classifier reads the [CLS] row of the last layer alone (pooler: hidden_states[:, 0]), and nothing after the last layer's
    // attention mixes tokens. So in the LAST layer of a classifier only the first 16-query block of every pair goes through
    // attention, and out-projection, FFN and both LayerNorms run on ONE row per pair (gathered into compact tensors): the same
    // arithmetic on the rows that are read, nothing computed for the rows that are not - 4.6M rows become 25,600 for a third of
    // the layer's kernels. An embedding model (mean pooling over all tokens) takes the full path.
    bool cls_tail = false;
    for (int l = 0; l < m->cfg.layers; ++l) {
        const auto& ly = m->layers[l];
        cls_tail = !m->embed && l == m->cfg.layers - 1;
        if (cls_tail) {                                                // K and V for every token, Q for the [CLS] rows alone
            launch(mx_gather_rows_kernel, gather_grid, dim3(256), 0, st, w.x8, nullptr, io.row_off, P, H / 32, w.xc8, nullptr, w.m_cls);
            mx_qkv(h, m, ly, st, 1, 2, w.x8, io.m_packed);
            mx_qkv(h, m, ly, st, 0, 1, w.xc8, w.m_cls, io.pair_off, P);
        } else
            mx_qkv(h, m, ly, st, 0, 3, w.x8, io.m_packed);
        // one 16-query block per wave up to L = 256 (16 waves per (head, pair)): same-box A/B against two blocks per wave: -2.6 % (four: +9 %)
        const int qblocks = cls_tail ? 1 : 1 << 20;
        rc = L <= 256 ? launch_attention<1, true>(h, m, w, w.qf16, w.kf16, w.vf16, ctx, c, st, qblocks)
                      : launch_attention<2, true>(h, m, w, w.qf16, w.kf16, w.vf16, ctx, c, st, qblocks);
        if (rc) return rc;
        if (cls_tail) {
            launch(mx_gather_rows_kernel, gather_grid, dim3(256), 0, st, w.ctx8, nullptr, io.row_off, P, H / 32, w.cc8, nullptr, w.m_cls);
            mx_layer_tail(h, m, ly, st, w.cc8, w.xc8, w.hc8, w.m_cls);
        } else
            mx_layer_tail(h, m, ly, st, w.ctx8, w.x8, w.h8, io.m_packed);
    }
    // head. After a [CLS] tail the classifier's rows are the compact tensor (row p = pair p), else row row_off[p] of the stream. (An
    // embedding model's row_off is its pair_off: its heads below read the stream through either.)
    const char* const cls = cls_tail ? w.xc8 : w.x8;
    if (m->embed) {
        if (c.out)
            launch(ce_meanpool_kernel<true>, dim3(P), dim3(256), 0, st, reinterpret_cast<const half_t*>(w.x8.get()), io.pair_off, io.clen, L, H,
                   m->normalize, m->pool_cls, c.out);
        if (c.lex || c.tok) {                                          // the heads read the split layout: rewrite the final image once
            launch(m3_mx_to_split_kernel, dim3((unsigned)(((int64_t)P * L * H + 255) / 256)), dim3(256), 0, st, w.x8, io.m_packed, H, m->heads.x16);
            if ((rc = heads_chunk(h, m, w, m->heads.x16, c, st))) return rc;
        }
    } else if (cls_tail && P >= 512)
        // the batched pooler pays from ~512 pairs on; a single query's 100 pairs fill more CUs with one workgroup per pair
        launch(mx_pool_classify_kernel, dim3((unsigned)((P + POOL_PB - 1) / POOL_PB)), dim3(256), 0, st, cls, m->wpT, m->bp, m->wc, m->bc, P, H, c.out);
    else
        launch(ce_pool_classify_kernel<true>, dim3(P), dim3(256), 0, st, reinterpret_cast<const half_t*>(cls), m->wp, m->bp, m->wc, m->bc,
               cls_tail ? nullptr : io.row_off.get(), H, c.out);
    HIP_TRY(h, hipGetLastError());
    return RAG_OK;
}

// Which forward: the MX kernels (hi16 + lo8 operands, 384 x 128 tiles; ce_mx.h) whenever the SHAPE allows (hidden 384, ffn a multiple
// of 384) and the load-time probe saw them within CE_PROBE_TOL of the split-fp16 forward, the split-fp16 kernels for every other
// model. By model alone, never by batch size: a pair's logit must not depend on how a batch was split over ranks or chunks.
// Option ce_mx: -1 = never, 1 = by shape (probe ignored), 0 = by shape and probe.
static bool ce_use_mx(const rag_ctx* h, const rag_ce_model* m) {
    return m->mx_ok && (h->opt.ce_mx > 0 || (h->opt.ce_mx == 0 && m->mx_default));
}

// Scratch of the heads for a workspace of `tokens` padded rows (a reallocation waits for st first, as ws_renew does)
static int heads_ensure_ws(rag_ctx* h, rag_ce_model* m, int64_t tokens, bool use_mx, bool tok, hipStream_t st) {
    ce_heads& hd = m->heads;
    const size_t H = m->cfg.hidden;
    int rc;
    if (use_mx && hd.x16_tokens != tokens) {
        HIP_TRY(h, hipStreamSynchronize(st));
        hd.x16_tokens = 0;
        if ((rc = alloc_zeroed(h, hd.x16, 2 * (size_t)tokens * H, st))) return rc;      // rows past the packed rows are GEMM operands: finite
        hd.x16_tokens = tokens;
    }
    if (tok && hd.raw_tokens != tokens) {
        HIP_TRY(h, hipStreamSynchronize(st));
        hd.raw_tokens = 0;
        if ((rc = hd.raw.alloc(h, (size_t)tokens * hd.tok_pad))) return rc;
        hd.raw_tokens = tokens;
    }
    return RAG_OK;
}

// out: [P][m->out_width] floats (logits of a cross-encoder, pooled vectors of an embedding model)
static int ce_run(rag_ctx* h, rag_ce_model* m, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L_in, float* out,
                  hipStream_t st, bool host_ptrs, bool use_mx, const ce_multi* mo = nullptr) {
    // mo (rag_embed_multi_*, device pointers only): the heads' outputs beside `out`, which may then be null
    ARG_CHECK(h, ids && tt && lens && (out || mo) && P > 0 && L_in > 0 && !(mo && host_ptrs), "ce_score: bad arguments");
    const size_t ow = (size_t)m->out_width;
    // the cut is made here, per call, never at load: min(max_pos, 512 with 32-wide heads, 8192 with 64-wide heads)
    if (L_in > ce_seq_limit(m)) {
        const int wl = ce_width_limit(m->d_head);
        h->err = "bad argument: ce_score: seq_len " + std::to_string(L_in) + " is past the model's limit of " + std::to_string(ce_seq_limit(m)) +
                 (m->cfg.max_pos < wl ? " tokens, set by max_position_embeddings (max_pos " + std::to_string(m->cfg.max_pos) + ")"
                                      : " tokens, set by the head width (" + std::to_string(m->d_head) + "-wide heads: " + std::to_string(wl) + ")");
        return RAG_ERR_ARG;
    }
    const int L = ce_length_class(m->d_head, L_in);
    // ~2M tokens of activations per chunk (~30 GB). Option ce_chunk_tokens (diagnostic) shrinks it so that parity tests can run
    // the multi-chunk loop on small inputs.
    const int64_t chunk_tokens = h->opt.ce_chunk_tokens >= 32 ? h->opt.ce_chunk_tokens : 2'000'000;
    // equal chunks: 25,600 pairs at L = 256 go as 4 x 6,400 and not 3 x 7,812 + 2,164 (a small last chunk leaves the persistent
    // GEMM workgroups of its one-feature-tile kernels 12-or-13 tiles each: 6 % of that chunk idle)
    const int chunk_max = std::max(1, std::min(P, (int)(chunk_tokens / L)));
    const int chunk = (P + (P + chunk_max - 1) / chunk_max - 1) / ((P + chunk_max - 1) / chunk_max);
    // the forward, chosen once: its workspace and its two functions
    const ce_chunk_bufs& io = use_mx ? m->mx.io : m->split.io;
    const auto ensure_ws = use_mx ? mx_ensure_ws : ce_ensure_ws;
    const auto forward_chunk = use_mx ? mx_forward_chunk : ce_forward_chunk;
    int rc = ensure_ws(h, m, chunk, L, st);
    if (rc) return rc;
    if (mo) {
        if ((rc = heads_ensure_ws(h, m, use_mx ? m->mx.tokens : m->split.tokens, use_mx, mo->tok != nullptr, st))) return rc;
        if (mo->row_off) launch(m3_row_off_kernel, dim3(1), dim3(1024), 0, st, lens, P, L_in, mo->row_off);
    }
    const hipMemcpyKind kin = hipMemcpyHostToDevice, kout = hipMemcpyDeviceToHost;
    if ((rc = prof_begin(h, 2, st))) return rc;
    for (int p0 = 0; p0 < P; p0 += chunk) {
        const int pc = std::min(chunk, P - p0);
        // host arrays are staged chunk by chunk; device arrays are read (ids, lens) and written (logits) where they are: four
        // small copies less per chunk, 45 us of a single-query call
        ce_chunk c = {ids + (size_t)p0 * L_in, tt + (size_t)p0 * L_in, lens + p0, out ? out + (size_t)p0 * ow : nullptr, pc, L_in, L};
        if (mo) {
            c.lex = mo->lex ? mo->lex + (size_t)p0 * L_in : nullptr;
            c.tok = mo->tok;
            c.row_off = mo->row_off ? mo->row_off + p0 : nullptr;
            c.tok_cap = mo->tok_cap;
        }
        if (host_ptrs) {
            HIP_TRY(h, hipMemcpyAsync(io.sid, c.ids, (size_t)pc * L_in * 4, kin, st));
            HIP_TRY(h, hipMemcpyAsync(io.stt, c.tt, (size_t)pc * L_in * 4, kin, st));
            HIP_TRY(h, hipMemcpyAsync(io.lens, c.lens, (size_t)pc * 4, kin, st));
            c.ids = io.sid; c.tt = io.stt; c.lens = io.lens; c.out = io.logits;
        }
        rc = forward_chunk(h, m, c, st);
        if (rc) break;
        if (host_ptrs) HIP_TRY(h, hipMemcpyAsync(out + (size_t)p0 * ow, io.logits, (size_t)pc * ow * 4, kout, st));
    }
    if (!rc) rc = prof_end(h, 2, st);
    // device-pointer calls stay asynchronous on the caller's stream (all buffers belong to the model workspace);
    // host-pointer calls return results, so they wait
    hipError_t e = host_ptrs ? hipStreamSynchronize(st) : hipGetLastError();
    if (rc) return rc;
    if (e != hipSuccess) {
        h->err = std::string("ce_score: ") + hipGetErrorString(e);
        return RAG_ERR_HIP;
    }
    return RAG_OK;
}

int ce_score(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L_in, float* out,
             hipStream_t st, bool host_ptrs) {
    ARG_CHECK(h, h->ce != nullptr, "no cross-encoder loaded");
    return ce_run(h, h->ce, ids, tt, lens, P, L_in, out, st, host_ptrs, ce_use_mx(h, h->ce));
}

int embed_run(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L_in, float* out, hipStream_t st,
              bool host_ptrs) {
    ARG_CHECK(h, h->emb != nullptr, "no embedding model loaded");
    return ce_run(h, h->emb, ids, tt, lens, P, L_in, out, st, host_ptrs, ce_use_mx(h, h->emb));
}

// ---- the embedder's optional heads ---------------------------------------------------------------------------------------
// tok_w [tok_dim][hidden] (+ tok_b [tok_dim] or null = 0) and / or lex_w [hidden] (+ lex_b): float32 host arrays. The token matrix
// is stored in the GEMM's split layout with its rows zero-padded to a multiple of 128 (one feature tile). A head that is not
// given stays as it was.
int embed_heads_load_host(rag_ctx* h, const float* tok_w, const float* tok_b, int tok_dim, const float* lex_w, float lex_b) {
    if (!h->emb) {
        h->err = "embed_heads_load: no embedding model loaded";
        return RAG_ERR_STATE;
    }
    ARG_CHECK(h, tok_w || lex_w, "embed_heads_load: neither head given");
    ARG_CHECK(h, !tok_w || (tok_dim >= 32 && tok_dim <= 1024 && tok_dim % 32 == 0), "embed_heads_load: tok_dim must be a multiple of 32 in [32, 1024]");
    rag_ce_model* m = h->emb;
    ce_heads& hd = m->heads;
    const size_t H = m->cfg.hidden;
    int rc;
    if (tok_w) {
        const int pad = (int)round_up(tok_dim, CE_BM);
        std::vector<float> wp((size_t)pad * H, 0.f), bp((size_t)pad, 0.f);
        std::memcpy(wp.data(), tok_w, (size_t)tok_dim * H * sizeof(float));
        if (tok_b) std::memcpy(bp.data(), tok_b, (size_t)tok_dim * sizeof(float));
        hd.tok_dim = hd.tok_pad = 0;
        hd.raw = dev_buf<float>();
        hd.raw_tokens = 0;
        dev_buf<char> none;
        if ((rc = up_weight(h, {wp.data()}, (size_t)pad, H, hd.tok_w, none, false))) return rc;      // waits: wp may go
        if ((rc = up_f32(h, bp.data(), (size_t)pad, hd.tok_b))) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        hd.tok_dim = tok_dim;
        hd.tok_pad = pad;
    }
    if (lex_w) {
        hd.lex_w = dev_buf<float>();
        dev_buf<float> w;
        if ((rc = up_f32(h, lex_w, H, w))) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        hd.lex_w = std::move(w);
        hd.lex_b = lex_b;
    }
    return RAG_OK;
}

// One forward, up to three outputs (each may be null). Device pointers, queued on st. row_off_out [P + 1] is filled whenever it is
// given; rows at or past tok_rows_cap are dropped.
static int embed_multi_dev_run(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L_in, float* dense, float* lex,
                               float* tok, int64_t tok_rows_cap, int64_t* row_off, hipStream_t st) {
    rag_ce_model* m = h->emb;
    ce_multi mo = {lex, tok, row_off, tok_rows_cap};
    return ce_run(h, m, ids, tt, lens, P, L_in, dense, st, false, ce_use_mx(h, m), &mo);
}

static int embed_multi_check(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L_in, const float* dense,
                             const float* lex, const float* tok, int64_t tok_rows_cap, const int64_t* row_off) {
    ARG_CHECK(h, ids && tt && lens && P > 0 && L_in > 0, "embed_multi: bad arguments");
    ARG_CHECK(h, dense || lex || tok, "embed_multi: no output asked for");
    ARG_CHECK(h, !tok || (row_off && tok_rows_cap >= 0), "embed_multi: token vectors need row_off_out and a capacity >= 0");
    if (!h->emb) {
        h->err = "embed_multi: no embedding model loaded";
        return RAG_ERR_STATE;
    }
    if ((tok && h->emb->heads.tok_dim == 0) || (lex && !h->emb->heads.lex_w)) {
        h->err = std::string("embed_multi: the ") + (tok && h->emb->heads.tok_dim == 0 ? "token-vector" : "lexical") + " head is not loaded (rag_embed_heads_load_host)";
        return RAG_ERR_STATE;
    }
    return RAG_OK;
}

int embed_multi_dev(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L_in, float* dense, float* lex, float* tok,
                    int64_t tok_rows_cap, int64_t* row_off, hipStream_t st) {
    if (int rc = embed_multi_check(h, ids, tt, lens, P, L_in, dense, lex, tok, tok_rows_cap, row_off)) return rc;
    return embed_multi_dev_run(h, ids, tt, lens, P, L_in, dense, lex, tok, tok_rows_cap, row_off, st);
}

// Host arrays: the row total is known before anything is queued, so a capacity that is too small is an error here. Inputs and
// outputs are staged in buffers of the call's own, which the device-pointer path then runs on; the call waits.
int embed_multi_host(rag_ctx* h, const int32_t* ids, const int32_t* tt, const int32_t* lens, int P, int L_in, float* dense, float* lex, float* tok,
                     int64_t tok_rows_cap, int64_t* row_off) {
    int rc;
    if ((rc = embed_multi_check(h, ids, tt, lens, P, L_in, dense, lex, tok, tok_rows_cap, row_off))) return rc;
    const rag_ce_model* m = h->emb;
    int64_t total = 0;
    for (int p = 0; p < P; ++p) total += std::max(1, std::min(lens[p], L_in)) - 1;
    ARG_CHECK(h, !tok || total <= tok_rows_cap, "embed_multi: tok_rows_cap is smaller than the call's token rows");
    const size_t H = m->cfg.hidden, D = m->heads.tok_dim, n_tok = (size_t)P * L_in;
    hipStream_t st = h->stream;
    dev_buf<int32_t> d_ids, d_tt, d_lens;
    dev_buf<float> d_dense, d_lex, d_tok;
    dev_buf<int64_t> d_off;
    if ((rc = d_ids.alloc(h, n_tok)) || (rc = d_tt.alloc(h, n_tok)) || (rc = d_lens.alloc(h, (size_t)P))) return rc;
    if (dense && (rc = d_dense.alloc(h, (size_t)P * H))) return rc;
    if (lex && (rc = d_lex.alloc(h, n_tok))) return rc;
    if (tok && (rc = d_tok.alloc(h, (size_t)std::max<int64_t>(total, 1) * D))) return rc;
    if (row_off && (rc = d_off.alloc(h, (size_t)P + 1))) return rc;
    HIP_TRY(h, hipMemcpyAsync(d_ids, ids, n_tok * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(d_tt, tt, n_tok * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(d_lens, lens, (size_t)P * 4, hipMemcpyHostToDevice, st));
    rc = embed_multi_dev_run(h, d_ids, d_tt, d_lens, P, L_in, d_dense, d_lex, d_tok, total, d_off, st);
    if (!rc && dense) HIP_TRY(h, hipMemcpyAsync(dense, d_dense, (size_t)P * H * 4, hipMemcpyDeviceToHost, st));
    if (!rc && lex) HIP_TRY(h, hipMemcpyAsync(lex, d_lex, n_tok * 4, hipMemcpyDeviceToHost, st));
    if (!rc && tok && total > 0) HIP_TRY(h, hipMemcpyAsync(tok, d_tok, (size_t)total * D * 4, hipMemcpyDeviceToHost, st));
    if (!rc && row_off) HIP_TRY(h, hipMemcpyAsync(row_off, d_off, ((size_t)P + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));                   // also before the staging buffers go
    return rc;
}

// Load-time accuracy probe of a classifier's MX forward. Its 8-bit correction operands track the split-fp16 forward to ~1e-3 on
// models like the seeded and random-init ones, but sharp attention heads (large Q / K weights) or LayerNorm outlier dimensions
// push the MX logits past the 4e-3 bar (stress levels). A fixed batch goes through both forwards; when they
// differ by more than CE_PROBE_TOL, option ce_mx = 0 takes the split-fp16 forward for this model. The choice depends on the
// weights alone. Pairs that are not finite on either forward say nothing about precision and are skipped.
#define CE_PROBE_PAIRS 16
#define CE_PROBE_TOL 2.5e-3f
static int ce_probe_mx(rag_ctx* h, rag_ce_model* m) {
    const int P = CE_PROBE_PAIRS, L = std::min(128, m->cfg.max_pos), V = m->cfg.vocab_size;
    const int id0 = V > 2000 ? 1000 : 0;               // WordPiece vocabularies keep [unused] and special tokens below 1000
    std::vector<int32_t> ids((size_t)P * L, 0), tt((size_t)P * L, 0), lens(P);
    uint32_t s = 0x9E3779B9u;
    for (int p = 0; p < P; ++p) {
        lens[p] = std::max(1, L - p * L / P);
        for (int t = 0; t < lens[p]; ++t) {
            s = s * 1664525u + 1013904223u;
            ids[(size_t)p * L + t] = id0 + (int)((s >> 8) % (uint32_t)(V - id0));
            tt[(size_t)p * L + t] = 3 * t >= lens[p];
        }
    }
    std::vector<float> mx(P), sp(P);
    int rc = ce_run(h, m, ids.data(), tt.data(), lens.data(), P, L, mx.data(), h->stream, true, true);
    if (!rc) rc = ce_run(h, m, ids.data(), tt.data(), lens.data(), P, L, sp.data(), h->stream, true, false);
    m->split = ce_split_ws();                           // the next call sizes its workspace for its own batch
    m->mx = ce_mx_ws();
    if (rc) return rc;
    float d = 0.f;
    for (int p = 0; p < P; ++p)
        if (std::isfinite(mx[p]) && std::isfinite(sp[p])) d = std::max(d, std::fabs(mx[p] - sp[p]));
    m->mx_default = d <= CE_PROBE_TOL;
    return RAG_OK;
}

int embed_dim(const rag_ctx* h) { return h->emb ? h->emb->cfg.hidden : -1; }
int embed_tok_dim(const rag_ctx* h) { return h->emb ? h->emb->heads.tok_dim : -1; }
