"""Every entry writes only inside the caller's output arrays (include/rag_hip.h gives their sizes in prose only), and the entries
that read a caller's array 16 bytes at a time refuse an address that is not 16-byte aligned.

Every other GPU test gives each output an allocation of its own (torch: 512-byte granules; numpy: malloc slack), so an entry that
rounds Q, k, pool or n up to a tile, a wave or a vector width and writes the excess passes them all. Here every array an entry may
write lies between two guard bands (tests/guard_tools.py: each as long as the array and at least 64 KiB, filled with 0xA5, the
array one element past a 16-byte boundary), every guard byte is compared after the call, and the outputs must equal, bit for bit,
those of the same call on a fresh handle with ordinary allocations. Both calls run on the default stream and are synchronised.

Device outputs: the case builders of tests/test_stream_order_gpu.py (A) and tests/test_stream_order_resident_gpu.py (R) are run
with their `out` and torch.empty / torch.full / torch.zeros(device="cuda") replaced by the guarded allocator, so the outputs the
wrappers of optimized_rag_amd/_lib.py allocate themselves are guarded too. Each case runs at its table shape and at ragged shapes
(RAGGED_A, RAGGED_R: 3 queries, k 3, pool 7; 1 query, k 1 where the builder makes that cheap; 129 queries - one past a 128-query
tile - for the dense-backed searches). Not run: A's hybrid_rrf_dev-long_bm25_leg, the 100,000-row world built to time the join of
the two legs; rag_hybrid_rrf_dev is run by four other cases.
No entry refused 3 queries, k 3 or pool 7 (every bound is 0 < k <= pool), so no shape had to be raised to a floor.
Host outputs: optimized_rag_amd._lib sees a numpy whose empty / zeros / full / empty_like / zeros_like hand out guarded arrays
(numpy itself is not patched); every host entry that fills an array is driven once at a ragged shape (HOST_ENTRIES, _host_cases).
Alignment (ALIGNED_INPUTS): an otherwise valid call whose array starts one element late is refused with RAG_ERR_ARG and a message
that says "16-byte aligned", before anything is enqueued - the check is host code, no misaligned access is made on the device, the
shifted array is never read or written by anything - and the same call, aligned, then returns the bits of a fresh handle.
test_every_entry_that_writes_is_guarded_or_exempt (no GPU) holds the tables against the header: every entry with a pointer to
non-const other than the handle and `void* stream` is named by a case here - and each guarded run checks the entries it names
against those it really called - or stands in EXEMPT with its reason.

Found on the library as it stood: no overrun and no understated size; every guarded run passed at the first attempt. What
changed in the library is the alignment rule alone (include/rag_hip.h, "Alignment"; aligned16 in csrc/common.h).

Mutants, one line each, built aside and run once against the narrowest test:
  the padding loop of rerank_topk_kernel (pipeline.hip) running to i <= k
      FAILS test_device_outputs_stay_inside_their_arrays[A-rerank_topk_dev-ragged]: "device array #0 (3, 3) torch.int64 (72 bytes):
      8 guard bytes changed behind its end, the first at byte offset +0 from the array's end"
  the D2H copy of rows_out in dense_topk_host_entry (api.hip) one element longer
      FAILS test_host_outputs_stay_inside_their_arrays[dense_topk]: "host array #1 (3, 3) int32 (36 bytes): 4 guard bytes changed
      behind its end" (malloc rounds those 36 bytes to 40: in an array of its own the extra element lands in slack)
Neither was run against the whole file.
Measured on an MI355X, one run: the 229 tests of this file in 4.5 s behind one process start, 1.9 s of it the first test, which
builds A's world; none of the others above 0.06 s. The two stream-order files on the commit before this one, same machine, one
run each: tests/test_stream_order_gpu.py 117 tests in 41.6 s, tests/test_stream_order_resident_gpu.py 101 tests in 30.7 s (their
busy work is 200 ms per queued regime; nothing here waits).
"""
import ctypes as C

import numpy as np
import pytest

import guard_tools as GT
import stream_tools as T
import test_stream_order_gpu as A
import test_stream_order_resident_gpu as R

gpu = pytest.mark.gpu


# ---- handles ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def handles():
    """handles(A or R, parts, options): a fresh handle (three for R's "shards") loaded with the named parts of that module's world"""
    from optimized_rag_amd import RagEngine
    made = []

    def new(dim, options):
        eng = RagEngine(dim=dim, device=0)
        made.append(eng)
        for name, value in options.items():
            eng.set_option(name, value)
        return eng

    def make(mod, parts, options):
        if mod is R:
            dim = R.DE if "embedder" in parts else R.D
            if "shards" in parts:
                return [R.load(new(dim, options), parts, lo, hi) for lo, hi in R.BOUNDS]
            return R.load(new(dim, options), parts)
        w = A.world()
        eng = new(A.CE_CFG["hidden"] if "embed" in parts else A.D, options)
        if "index" in parts:
            eng.index_load(w["emb"])
        if "bm25" in parts:
            w["post"].load(eng)
        if "temporal" in parts:
            eng.set_temporal(w["temporal"])
        if "ce" in parts:
            eng.ce_load(A.CE_CFG, w["ce_t"])
        if "embed" in parts:
            eng.embed_load(A.CE_CFG, w["emb_t"], normalize=True)
        if "tokens" in parts:
            eng.tokens_load(w["tok"], w["tok_len"])
        return eng

    yield make
    for e in made:
        e.close()


def record(engs, seen):
    for e in engs if isinstance(engs, list) else [engs]:
        e.lib = GT.Recorder(e.lib, seen)


def same_bits(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, f"{what} output {i}: {g.dtype} {g.shape} against {r.dtype} {r.shape}"
        if g.tobytes() != r.tobytes():
            diff = np.flatnonzero(g.reshape(-1).view(np.uint8) != r.reshape(-1).view(np.uint8))
            raise AssertionError(f"{what} output {i}: {diff.size} bytes differ from the unguarded call, the first at byte {int(diff[0])}")


# ---- 1. device outputs ------------------------------------------------------------------------------------------------------------------
SKIPPED_A = {"hybrid_rrf_dev-long_bm25_leg"}
ENTRIES_A = {name: ("rag_" + name.split("-")[0],) for name in A.CASES if name not in SKIPPED_A}
ENTRIES_A.update({
    "tokens_append_dev": ("rag_tokens_append_dev", "rag_ce_build_pairs_dev"),
    "index_load_dev": ("rag_index_load_dev", "rag_dense_topk_dev"),
    "index_append_dev": ("rag_index_append_dev", "rag_dense_topk_dev"),
})

# name of the case in A.CASES -> {shape name: builder}. 3 queries, k 3, pool 7; "one": 1 query, k 1; "q129": one query past a tile
RAGGED_A = {
    "dense_topk_dev": dict(ragged=lambda: A.case_dense(Q=3, k=3), one=lambda: A.case_dense(Q=1, k=1), q129=lambda: A.case_dense(Q=129, k=3)),
    "merge_topk_dev": dict(ragged=lambda: A.case_merge(L=3, Q=3, k=3), one=lambda: A.case_merge(L=2, Q=1, k=1)),
    "hybrid_fuse_gathered_dev": dict(ragged=lambda: A.case_fuse_gathered(W=2, Q=3, pool=7, k=3), one=lambda: A.case_fuse_gathered(W=1, Q=1, pool=7, k=1)),
    "rrf_fuse_dev": dict(ragged=lambda: A.case_rrf(Q=3, n_lists=2, ln=7, k=3), one=lambda: A.case_rrf(Q=1, n_lists=3, ln=7, k=1)),
    "bm25_topk_dev": dict(ragged=lambda: A.case_bm25(Q=3, k=3), one=lambda: A.case_bm25(Q=1, k=1)),
    "bm25_topk_dev-sub_batched": dict(ragged=lambda: A.case_bm25(Q=3, k=3, bm25_ws_mb=1)),
    "hybrid_rrf_dev-forked": dict(ragged=lambda: A.case_hybrid_rrf(Q=3, pool=7, k=3), one=lambda: A.case_hybrid_rrf(Q=1, pool=7, k=1),
                                  q129=lambda: A.case_hybrid_rrf(Q=129, pool=7, k=3)),
    "hybrid_rrf_dev-no_fork": dict(ragged=lambda: A.case_hybrid_rrf(Q=3, pool=7, k=3, no_fork=1)),
    "hybrid_rrf_dev-above_fork_max_q": dict(q129=lambda: A.case_hybrid_rrf(Q=129, pool=7, k=3, fork_max_q=100)),
    "hybrid_rrf_dev-below_fork_max_q": dict(ragged=lambda: A.case_hybrid_rrf(Q=3, pool=7, k=3, fork_max_q=100)),
    "hybrid_linear_dev": dict(ragged=lambda: A.case_hybrid_linear(Q=3, k=3), one=lambda: A.case_hybrid_linear(Q=1, k=1),
                              q129=lambda: A.case_hybrid_linear(Q=129, k=3)),
    "mmr_select_dev-0": dict(ragged=lambda: A.case_mmr(0, Q=3, pool=7, k=3), one=lambda: A.case_mmr(0, Q=1, pool=7, k=1)),
    "mmr_select_dev-1": dict(ragged=lambda: A.case_mmr(1, Q=3, pool=7, k=3)),
    "ce_score_dev-mx": dict(ragged=lambda: A.case_ce(1, P=3, L=64), one=lambda: A.case_ce(1, P=1, L=64)),
    "ce_score_dev-split": dict(ragged=lambda: A.case_ce(-1, P=3, L=64)),
    "embed_dev": dict(ragged=lambda: A.case_embed(P=3, L=64), one=lambda: A.case_embed(P=1, L=64)),
    "ce_build_pairs_dev": dict(ragged=lambda: A.case_build_pairs(Q=3, pool=7, Lq=6, L=33), one=lambda: A.case_build_pairs(Q=1, pool=7, Lq=6, L=9)),
    "rerank_topk_dev": dict(ragged=lambda: A.case_rerank_topk(Q=3, pool=7, k=3), one=lambda: A.case_rerank_topk(Q=1, pool=7, k=1)),
    "retrieve_rerank_dev-0": dict(ragged=lambda: A.case_retrieve_rerank(0, Q=3, pool=7, k=3), one=lambda: A.case_retrieve_rerank(0, Q=1, pool=7, k=1)),
    "retrieve_rerank_dev-1": dict(ragged=lambda: A.case_retrieve_rerank(1, Q=3, pool=7, k=3)),
}
# R's builders read POOL and K from their module: the ragged runs set them to 7 and 3 ("one": k 1) for the length of the test
RAGGED_R = {
    "dense_topk_tenants_dev": dict(ragged=lambda: R.case_dense_tenants(n=3), one=lambda: R.case_dense_tenants(n=1), q129=lambda: R.case_dense_tenants(n=129)),
    "sparse_topk_dev": dict(ragged=lambda: R.case_sparse_topk(n=3), one=lambda: R.case_sparse_topk(n=1)),
    "sparse_topk_tenants_dev": dict(ragged=lambda: R.case_sparse_topk(True, n=3)),
    "bm25_topk_tenants_dev": dict(ragged=lambda: R.case_bm25(n=3), one=lambda: R.case_bm25(n=1)),
    "hybrid_rrf_tenants_dev": dict(ragged=lambda: R.case_hybrid_rrf(n=3), q129=lambda: R.case_hybrid_rrf(n=129)),
    "hybrid_sparse_rrf_dev-forked": dict(ragged=lambda: R.case_hybrid_sparse_rrf(n=3), one=lambda: R.case_hybrid_sparse_rrf(n=1),
                                         q129=lambda: R.case_hybrid_sparse_rrf(n=129)),
    "hybrid_sparse_rrf_dev-no_fork": dict(ragged=lambda: R.case_hybrid_sparse_rrf(n=3, no_fork=1)),
    "hybrid_sparse_rrf_tenants_dev": dict(ragged=lambda: R.case_hybrid_sparse_rrf(True, n=3), q129=lambda: R.case_hybrid_sparse_rrf(True, n=129)),
    "hybrid_linear_tenants_dev": dict(ragged=lambda: R.case_hybrid_linear_tenants(n=3), q129=lambda: R.case_hybrid_linear_tenants(n=129)),
    "retrieve_rerank_tenants_dev": dict(ragged=lambda: R.case_retrieve_rerank_tenants(n=3, pool=7, k=3)),
    "sparse_score_rows_dev": dict(ragged=lambda: R.case_sparse_score_rows(n=3), one=lambda: R.case_sparse_score_rows(n=1)),
    "m3_score_rows_dev-three_way": dict(ragged=lambda: R.case_m3_score_rows(R.W3, n=3), one=lambda: R.case_m3_score_rows(R.W3, n=1)),
    "m3_score_rows_dev-colbert_only": dict(ragged=lambda: R.case_m3_score_rows((0.0, 0.0, 1.0), n=3)),
    "tokvec_rerank_dev-fp16": dict(ragged=lambda: R.case_tokvec_rerank(n=3), one=lambda: R.case_tokvec_rerank(n=1)),
    "tokvec_rerank_dev-mxfp8": dict(ragged=lambda: R.case_tokvec_rerank("tokvec8", n=3)),
    "retrieve_maxsim_dev": dict(ragged=lambda: R.case_retrieve_maxsim(n=3), q129=lambda: R.case_retrieve_maxsim(n=129)),
    "retrieve_maxsim_tenants_dev": dict(ragged=lambda: R.case_retrieve_maxsim(True, n=3)),
    "retrieve_m3_dev-0": dict(ragged=lambda: R.case_retrieve_m3(0, n=3)),
    "retrieve_m3_dev-1": dict(ragged=lambda: R.case_retrieve_m3(1, n=3)),
    "retrieve_m3_dev-2": dict(ragged=lambda: R.case_retrieve_m3(2, n=3), one=lambda: R.case_retrieve_m3(2, n=1), q129=lambda: R.case_retrieve_m3(2, n=129)),
    "retrieve_m3_tenants_dev": dict(ragged=lambda: R.case_retrieve_m3(2, True, n=3)),
    "maxsim_dev": dict(ragged=lambda: R.case_maxsim(n=3, n_docs=5, n_pairs=7), one=lambda: R.case_maxsim(n=1, n_docs=1, n_pairs=1)),
    "lexical_match_dev": dict(ragged=lambda: R.case_lexical_match(n=3, n_pairs=7), one=lambda: R.case_lexical_match(n=1, n_pairs=1)),
    "lexical_compact_dev": dict(ragged=lambda: R.case_lexical_compact(n=3), one=lambda: R.case_lexical_compact(n=1)),
    "embed_multi_dev": dict(ragged=lambda: R.case_embed_multi(n=3), one=lambda: R.case_embed_multi(n=1)),
    "search_m3_tokens_dev": dict(ragged=lambda: R.case_search_m3_tokens(n=3), one=lambda: R.case_search_m3_tokens(n=1)),
    "search_m3_tokens_tenants_dev": dict(ragged=lambda: R.case_search_m3_tokens(True, n=3)),
    "rows_of_ids_dev": dict(ragged=lambda: R.case_rows_of_ids(n=7), one=lambda: R.case_rows_of_ids(n=1)),
    "m3_candidates_gathered_dev-0": dict(ragged=lambda: R.case_m3_candidates_gathered(0, n=3)),
    "m3_candidates_gathered_dev-1": dict(ragged=lambda: R.case_m3_candidates_gathered(1, n=3)),
    "m3_candidates_gathered_dev-2": dict(ragged=lambda: R.case_m3_candidates_gathered(2, n=3), one=lambda: R.case_m3_candidates_gathered(2, n=1)),
    "m3_score_ids_dev-implicit_ids": dict(ragged=lambda: R.case_m3_score_ids(False, n=3, width=14)),
    "m3_score_ids_dev-explicit_ids": dict(ragged=lambda: R.case_m3_score_ids(True, n=3, width=14), one=lambda: R.case_m3_score_ids(True, n=1, width=7)),
    "m3_combine_gathered_dev": dict(ragged=lambda: R.case_m3_combine_gathered(n=3, width=14), one=lambda: R.case_m3_combine_gathered(n=1, width=7)),
    "m3_shard_chain": dict(ragged=lambda: R.case_shard_chain(2, n=3)),
    "hybrid_linear_chain": dict(ragged=lambda: R.case_linear_chain(n=3), one=lambda: R.case_linear_chain(n=1)),
    "hybrid_linear_chain-tenants": dict(ragged=lambda: R.case_linear_chain(True, n=3)),
    "tokvec_append_dev": dict(ragged=lambda: R.case_tokvec_append(n=7)),
    "sparse_append_dev": dict(ragged=lambda: R.case_sparse_append(n=7)),
}
DEVICE_RUNS = [("A", name, "table") for name in sorted(ENTRIES_A)] + [("A", name, shape) for name in sorted(RAGGED_A) for shape in RAGGED_A[name]] + \
              [("R", name, "table") for name in sorted(R.CASES)] + [("R", name, shape) for name in sorted(RAGGED_R) for shape in RAGGED_R[name]]


def device_case(monkeypatch, which, name, shape):
    """(module, the Case at that shape, the *_dev entries it must reach)"""
    mod = A if which == "A" else R
    entries = ENTRIES_A[name] if mod is A else R.ENTRIES[name]
    if shape == "table":
        return mod, mod.CASES[name][0](), entries
    if mod is R:
        monkeypatch.setattr(R, "POOL", 7)
        monkeypatch.setattr(R, "K", 1 if shape == "one" else 3)
    return mod, (RAGGED_A if mod is A else RAGGED_R)[name][shape](), entries


def guard_device(monkeypatch, guards):
    """from here to the end of the test: `out` of both modules and torch's three allocators hand out guarded device arrays"""
    GT.patch_torch(monkeypatch, guards)

    def out(shape, dtype, fill=-7):
        return guards.dev(shape, dtype, fill=fill)
    monkeypatch.setattr(A, "out", out)
    monkeypatch.setattr(R, "out", out)


@gpu
@pytest.mark.parametrize("which,name,shape", DEVICE_RUNS, ids=["-".join(r) for r in DEVICE_RUNS])
def test_device_outputs_stay_inside_their_arrays(handles, monkeypatch, which, name, shape):
    """The call with every output between guard bands: no guard byte changes, the outputs are those of a fresh handle with ordinary
    allocations, and the case reached the entries it stands for."""
    import torch
    mod, case, entries = device_case(monkeypatch, which, name, shape)
    ref = T.to_np(case.bind(handles(mod, case.parts, case.options))(T.to_dev(case.real), None))
    torch.cuda.synchronize()
    eng = handles(mod, case.parts, case.options)
    seen = set()
    record(eng, seen)
    call = case.bind(eng)
    dev = T.to_dev(case.real)
    torch.cuda.synchronize()
    guards = GT.Guards()
    guard_device(monkeypatch, guards)
    outs = call(dev, None)
    assert guards.check() >= len(outs), "the outputs were not allocated under guards"
    same_bits(T.to_np(outs), ref, f"{name} {shape}")
    assert {s for s in seen if s.endswith("_dev")} == set(entries), f"{name} reached {sorted(seen)}"


# ---- 3. alignment -------------------------------------------------------------------------------------------------------------------
# (module, case name, builder at the ragged shape, the input of the Case that is the array, what the message must name)
ALIGNED_INPUTS = [
    ("A", "dense_topk_dev", lambda: A.case_dense(Q=3, k=3), "q", "q_dev"),
    ("R", "dense_topk_tenants_dev", lambda: R.case_dense_tenants(n=3), "q", "q_dev"),
    ("A", "hybrid_rrf_dev-forked", lambda: A.case_hybrid_rrf(Q=3, pool=7, k=3), "q", "q_dev"),
    ("R", "hybrid_rrf_tenants_dev", lambda: R.case_hybrid_rrf(n=3), "q", "q_dev"),
    ("R", "hybrid_sparse_rrf_dev-forked", lambda: R.case_hybrid_sparse_rrf(n=3), "q", "q_dev"),
    ("R", "hybrid_sparse_rrf_tenants_dev", lambda: R.case_hybrid_sparse_rrf(True, n=3), "q", "q_dev"),
    ("A", "hybrid_linear_dev", lambda: A.case_hybrid_linear(Q=3, k=3), "q", "q_dev"),
    ("R", "hybrid_linear_tenants_dev", lambda: R.case_hybrid_linear_tenants(n=3), "q", "q_dev"),
    ("R", "hybrid_linear_chain", lambda: R.case_linear_chain(n=3), "q", "hybrid_linear_finish: the queries (q_dev)"),
    ("R", "hybrid_linear_chain-tenants", lambda: R.case_linear_chain(True, n=3), "q", "hybrid_linear_finish: the queries (q_dev)"),
    ("A", "retrieve_rerank_dev-0", lambda: A.case_retrieve_rerank(0, Q=3, pool=7, k=3), "q", "q_emb_dev"),
    ("A", "retrieve_rerank_dev-1", lambda: A.case_retrieve_rerank(1, Q=3, pool=7, k=3), "q", "q_emb_dev"),
    ("R", "retrieve_rerank_tenants_dev", lambda: R.case_retrieve_rerank_tenants(n=3, pool=7, k=3), "q", "q_emb_dev"),
    ("R", "retrieve_maxsim_dev", lambda: R.case_retrieve_maxsim(n=3), "q", "q_emb_dev"),
    ("R", "retrieve_maxsim_dev", lambda: R.case_retrieve_maxsim(n=3), "qv", "q_vecs_dev"),
    ("R", "retrieve_maxsim_tenants_dev", lambda: R.case_retrieve_maxsim(True, n=3), "q", "q_emb_dev"),
    ("R", "retrieve_maxsim_tenants_dev", lambda: R.case_retrieve_maxsim(True, n=3), "qv", "q_vecs_dev"),
    ("R", "retrieve_m3_dev-2", lambda: R.case_retrieve_m3(2, n=3), "q", "q_emb_dev"),
    ("R", "retrieve_m3_dev-2", lambda: R.case_retrieve_m3(2, n=3), "qv", "the query's token vectors"),
    ("R", "retrieve_m3_tenants_dev", lambda: R.case_retrieve_m3(2, True, n=3), "q", "q_emb_dev"),
    ("R", "m3_score_rows_dev-three_way", lambda: R.case_m3_score_rows(R.W3, n=3), "q", "the query embeddings"),
    ("R", "m3_score_rows_dev-three_way", lambda: R.case_m3_score_rows(R.W3, n=3), "qv", "the query's token vectors"),
    ("R", "m3_score_ids_dev-implicit_ids", lambda: R.case_m3_score_ids(False, n=3, width=14), "q", "the query embeddings"),
    ("R", "m3_score_ids_dev-implicit_ids", lambda: R.case_m3_score_ids(False, n=3, width=14), "qv", "the query's token vectors"),
    ("R", "tokvec_rerank_dev-fp16", lambda: R.case_tokvec_rerank(n=3), "qv", "query vectors"),
    ("R", "tokvec_rerank_dev-mxfp8", lambda: R.case_tokvec_rerank("tokvec8", n=3), "qv", "query vectors"),
    ("R", "maxsim_dev", lambda: R.case_maxsim(n=3, n_docs=5, n_pairs=7), "q", "vectors"),
    ("R", "maxsim_dev", lambda: R.case_maxsim(n=3, n_docs=5, n_pairs=7), "d", "vectors"),
]


@gpu
@pytest.mark.parametrize("which,name,builder,key,named", ALIGNED_INPUTS, ids=[f"{a[1]}-{a[3]}" for a in ALIGNED_INPUTS])
def test_an_array_read_16_bytes_at_a_time_must_be_16_byte_aligned(handles, monkeypatch, which, name, builder, key, named):
    """The array one element late: RAG_ERR_ARG, the message names it and says "16-byte aligned". The check runs on the host before
    any launch; the shifted array (zeros nobody reads) is never touched by the device. Aligned, the same handle then returns the
    bits of a fresh one."""
    import torch
    from optimized_rag_amd import RagError
    mod = A if which == "A" else R
    if mod is R:
        monkeypatch.setattr(R, "POOL", 7)
        monkeypatch.setattr(R, "K", 3)
    case = builder()
    ref = T.to_np(case.bind(handles(mod, case.parts, case.options))(T.to_dev(case.real), None))
    torch.cuda.synchronize()
    eng = handles(mod, case.parts, case.options)
    call = case.bind(eng)
    dev = T.to_dev(case.real)
    good = dev[key]
    assert good.data_ptr() % 16 == 0 and good.dtype == torch.float32
    late = torch.zeros(good.numel() + 1, dtype=good.dtype, device="cuda")[1:].view(good.shape)
    assert late.data_ptr() % 16 == good.element_size() and late.is_contiguous()
    torch.cuda.synchronize()
    with pytest.raises(RagError) as err:
        call(dict(dev, **{key: late}), None)
    assert "failed (-1): bad argument:" in str(err.value) and "16-byte aligned" in str(err.value) and named in str(err.value), str(err.value)
    torch.cuda.synchronize()
    same_bits(T.to_np(call(dev, None)), ref, f"{name}, aligned after the refusal")


# ---- 2. host outputs ------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _small_postings():
    from optimized_rag_amd.bm25 import Bm25Postings
    rng = _rng(41)
    post = Bm25Postings.from_corpus([" ".join(f"w{t}" for t in rng.integers(0, 30, 9)) for _ in range(37)])
    ptr, terms = post.encode_queries(["w1 w2 w29", "w5", "zzz w7 w7"])
    return post, ptr, terms


def _deleted(eng):
    """five rows gone: both ends of the index and both sides of a 2048-document range"""
    assert eng.index_delete(np.array([0, 5, 2047, 2048, R.N - 1])) == 5
    return eng


def _fetch(eng, doc):
    """the document through the wrapper (cap_rows = its rows), then with two rows of room to spare, then one row short (refused:
    the count is written, the array is not)"""
    from optimized_rag_amd import _lib
    out = eng.tokvec_fetch(doc)
    n, dim = out.shape
    assert n >= 2
    roomy, short, cnt = _lib.np.full((n + 2, dim), -3.0, dtype=np.float32), _lib.np.full((n - 1, dim), -3.0, dtype=np.float32), C.c_int64()
    assert eng.lib.rag_tokvec_fetch_host(eng.h, doc, _lib._ptr(roomy), n + 2, C.byref(cnt)) == 0 and cnt.value == n
    assert (roomy[:n] == out).all() and (roomy[n:] == -3.0).all()
    cnt.value = 0
    assert eng.lib.rag_tokvec_fetch_host(eng.h, doc, _lib._ptr(short), n - 1, C.byref(cnt)) == -1 and cnt.value == n
    assert (short == -3.0).all()
    return [out, roomy, short]


def _long_doc():
    off = R.world()["d_off"]
    return int(np.flatnonzero(np.diff(off[:200]) == 7)[0])             # 7 token vectors


def _host_cases():
    """name -> (the entries it stands for, parts of R's world, options, call(eng) -> list of arrays). Built on first use."""
    w = R.world()
    q3 = np.ascontiguousarray(w["q"][:3, :R.D])
    ten3 = np.array([0, 2, -1], np.int32)
    kw, lx, vq = R.keywords(3), R.lex(3), R.vecs(3)
    cand = R.slots(_rng(42), 3, 7)
    post, sptr, sterms = _small_postings()
    ints = __import__("small_inputs").int_vectors(_rng(43), 10, R.D)
    sents = __import__("small_inputs").clustered_sentences(_rng(44), 7, R.D)
    sent_len = _rng(45).integers(20, 200, 7).astype(np.int32)
    tx, (tok, _) = R.texts(3), R.token_inputs(3)
    pq, pd = _rng(46).integers(-1, 4, 7).astype(np.int32), _rng(47).integers(-1, 6, 7).astype(np.int32)
    docs5, off5 = np.array(w["d_vecs"][:w["d_off"][5]]), np.array(w["d_off"][:6])
    pairs = A.pairs(_rng(48), 3, 64)
    sem, key, tmp = _rng(49).random(37), _rng(50).random(37), _rng(51).random(37)
    doc = _long_doc()
    return {
        "dense_topk": (("rag_dense_topk_host",), ("index",), {}, lambda e: list(e.dense_topk(q3, 3))),
        "dense_topk_tenants": (("rag_dense_topk_tenants_host",), ("index", "tenants"), {}, lambda e: list(e.dense_topk(q3, 3, tenant=ten3))),
        "bm25_topk": (("rag_bm25_topk_host",), ("index", "bm25"), {}, lambda e: list(e.bm25_topk(kw["ptr"], kw["terms"], 3))),
        "bm25_topk_tenants": (("rag_bm25_topk_tenants_host",), ("index", "tenants", "bm25"), {},
                              lambda e: list(e.bm25_topk(kw["ptr"], kw["terms"], 3, tenant=ten3))),
        "sparse_topk": (("rag_sparse_topk_host",), ("index", "sparse"), {}, lambda e: list(e.sparse_topk(lx["ptr"], lx["terms"], lx["w"], 3))),
        "sparse_topk_tenants": (("rag_sparse_topk_tenants_host",), ("index", "tenants", "sparse"), {},
                                lambda e: list(e.sparse_topk(lx["ptr"], lx["terms"], lx["w"], 3, tenant=ten3))),
        "bm25_scores": (("rag_bm25_scores_host",), ("index", "bm25"), {}, lambda e: [e.bm25_scores(kw["ptr"], kw["terms"])]),
        "bm25_scores_adhoc": (("rag_bm25_scores_adhoc_host",), (), {},
                              lambda e: [e.bm25_scores_adhoc(post.indptr, post.doc, post.tf, post.doc_len, post.idf, post.avgdl, sptr, sterms)]),
        "sparse_scores": (("rag_sparse_scores_host",), ("index", "sparse"), {}, lambda e: [e.sparse_scores(lx["ptr"], lx["terms"], lx["w"])]),
        "sparse_score_rows": (("rag_sparse_score_rows_host",), ("index", "sparse"), {},
                              lambda e: [e.sparse_score_rows(lx["ptr"], lx["terms"], lx["w"], cand)]),
        "rrf_fuse": (("rag_rrf_fuse_host",), (), {}, lambda e: list(e.rrf_fuse(A.rrf_lists(_rng(52), 3, 2, 7), top_k=3))),
        "linear_fuse_topk": (("rag_linear_fuse_topk_host",), (), {}, lambda e: list(e.linear_fuse_topk(sem, key, tmp, 0.6, 0.3, 0.1, 3))),
        "mmr_select-0": (("rag_mmr_select_host",), (), {}, lambda e: list(e.mmr_select(ints[0], ints[1:8], 3, 0.7, 0))),
        "mmr_select-1": (("rag_mmr_select_host",), (), {}, lambda e: list(e.mmr_select(ints[0], ints[1:8], 3, 0.7, 1))),
        "chunk_chain": (("rag_chunk_chain_host",), (), {}, lambda e: [e.chunk_chain(sents, sent_len, 0.3, 400, 50)]),
        "pairwise_cosine": (("rag_pairwise_cosine_host",), (), {}, lambda e: [e.pairwise_cosine(ints[:3], ints[3:10])]),
        "pairwise_cosine_f64": (("rag_pairwise_cosine_f64_host",), (), {},
                                lambda e: [e.pairwise_cosine(ints[:3].astype(np.float64) / 3.0, ints[3:10].astype(np.float64) / 7.0)]),
        "ce_score": (("rag_ce_score_host",), ("ce",), {}, lambda e: [e.ce_score(pairs["ids"], pairs["tt"], pairs["lens"])]),
        "embed": (("rag_embed_host",), ("embedder",), {}, lambda e: [e.embed(tok["ids"], tok["tt"], tok["lens"])]),
        "embed_multi": (("rag_embed_multi_host",), ("embedder",), {}, lambda e: list(e.embed_multi(tok["ids"], tok["tt"], tok["lens"]))),
        "maxsim": (("rag_maxsim_host",), (), {}, lambda e: [e.maxsim(vq["qv"], vq["qo"], docs5, off5, pq, pd)]),
        "lexical_match": (("rag_lexical_match_host",), (), {},
                          lambda e: [e.lexical_match(tx["ids"], tx["w"], tx["lens"], tx["ids"], tx["w"], tx["lens"], pq, pq[::-1].copy(), skip_ids=R.SKIP)]),
        "lexical_compact": (("rag_lexical_compact_host",), (), {}, lambda e: list(e.lexical_compact(tx["ids"], tx["w"], tx["lens"], skip_ids=R.SKIP))),
        "tokvec_fetch-fp16": (("rag_tokvec_fetch_host",), ("index", "tokvec"), {}, lambda e: _fetch(e, doc)),
        "tokvec_fetch-mxfp8": (("rag_tokvec_fetch_host",), ("index", "tokvec8"), {}, lambda e: _fetch(e, doc)),
        "tokvec_rerank": (("rag_tokvec_rerank_host",), ("index", "tokvec"), {}, lambda e: list(e.tokvec_rerank(vq["qv"], vq["qo"], cand, 3))),
        "index_fetch_rows": (("rag_index_fetch_rows_host",), ("index",), {}, lambda e: [e.fetch_rows(np.array([0, R.N - 1, 17, 2048, 2047, 5, 5]))]),
        "rows_of_ids": (("rag_index_rows_of_ids_host",), ("ids",), {}, lambda e: [e.rows_of_ids(R.asked_ids(_rng(53), 7))]),
        "index_compact": (("rag_index_compact",), ("index",), {}, lambda e: [_deleted(e).index_compact()]),
        "index_compact_bm25": (("rag_index_compact_bm25",), ("index", "bm25"), {}, lambda e: [_deleted(e).index_compact(keep_postings=True)]),
        "index_compact_live": (("rag_index_compact_live",), ("index", "bm25", "sparse", "tokvec"), {},
                               lambda e: [_deleted(e).index_compact(keep_resident=True)]),
        "bm25_live_counts": (("rag_bm25_live_counts_host",), ("index", "bm25"), dict(bm25_keep_tf=1), lambda e: [_deleted(e).bm25_live_counts()[0]]),
        "bm25_refresh": (("rag_bm25_refresh",), ("index", "bm25"), dict(bm25_keep_tf=1), lambda e: [_deleted(e).bm25_refresh()[0]]),
        "sparse_export": (("rag_sparse_export_host",), ("index", "sparse"), {},
                          lambda e: [v for k, v in sorted(e.sparse_export().items()) if k != "n_docs"]),
    }


HOST_ENTRIES = {
    "dense_topk": ("rag_dense_topk_host",), "dense_topk_tenants": ("rag_dense_topk_tenants_host",), "bm25_topk": ("rag_bm25_topk_host",),
    "bm25_topk_tenants": ("rag_bm25_topk_tenants_host",), "sparse_topk": ("rag_sparse_topk_host",),
    "sparse_topk_tenants": ("rag_sparse_topk_tenants_host",), "bm25_scores": ("rag_bm25_scores_host",),
    "bm25_scores_adhoc": ("rag_bm25_scores_adhoc_host",), "sparse_scores": ("rag_sparse_scores_host",),
    "sparse_score_rows": ("rag_sparse_score_rows_host",), "rrf_fuse": ("rag_rrf_fuse_host",), "linear_fuse_topk": ("rag_linear_fuse_topk_host",),
    "mmr_select-0": ("rag_mmr_select_host",), "mmr_select-1": ("rag_mmr_select_host",), "chunk_chain": ("rag_chunk_chain_host",),
    "pairwise_cosine": ("rag_pairwise_cosine_host",), "pairwise_cosine_f64": ("rag_pairwise_cosine_f64_host",), "ce_score": ("rag_ce_score_host",),
    "embed": ("rag_embed_host",), "embed_multi": ("rag_embed_multi_host",), "maxsim": ("rag_maxsim_host",),
    "lexical_match": ("rag_lexical_match_host",), "lexical_compact": ("rag_lexical_compact_host",), "tokvec_fetch-fp16": ("rag_tokvec_fetch_host",),
    "tokvec_fetch-mxfp8": ("rag_tokvec_fetch_host",), "tokvec_rerank": ("rag_tokvec_rerank_host",), "index_fetch_rows": ("rag_index_fetch_rows_host",),
    "rows_of_ids": ("rag_index_rows_of_ids_host",), "index_compact": ("rag_index_compact",), "index_compact_bm25": ("rag_index_compact_bm25",),
    "index_compact_live": ("rag_index_compact_live",), "bm25_live_counts": ("rag_bm25_live_counts_host",), "bm25_refresh": ("rag_bm25_refresh",),
    "sparse_export": ("rag_sparse_export_host",),
}
GRID_PLAN = "rag_bm25_grid_plan"             # takes no handle: test_the_grid_plan_writes_five_numbers


@gpu
@pytest.mark.parametrize("name", sorted(HOST_ENTRIES))
def test_host_outputs_stay_inside_their_arrays(handles, monkeypatch, name):
    """The wrapper's own call, then the same call on a second fresh handle while the wrapper's numpy hands out guarded arrays: no
    guard byte changes, the results are the same bits, and the entries the case stands for were called."""
    from optimized_rag_amd import _lib
    entries, parts, options, call = _host_cases()[name]
    assert entries == HOST_ENTRIES[name]
    ref = call(handles(R, parts, options))
    eng = handles(R, parts, options)
    seen = set()
    record(eng, seen)
    guards = GT.Guards()
    monkeypatch.setattr(_lib, "np", GT.GuardedNumpy(guards))
    got = call(eng)
    assert guards.check() >= len(got), "the outputs were not allocated under guards"
    same_bits(got, ref, name)
    assert set(entries) <= seen, f"{name} reached {sorted(seen)}"


def test_the_table_of_host_cases_is_the_one_the_cases_are_built_from():
    """(no GPU) HOST_ENTRIES is what the completeness check reads; the cases themselves need R's world"""
    cases = _host_cases()
    assert {k: v[0] for k, v in cases.items()} == HOST_ENTRIES


def test_the_grid_plan_writes_five_numbers():
    """rag_bm25_grid_plan(out5) takes no handle and no GPU: called directly with a guarded int64[5], against the wrapper's tuple"""
    from optimized_rag_amd import _lib
    lib = _lib.load_library()
    for ranges, queries, linear in ((3, 3, 0), (1, 1, 1), (49, 129, 0), (4, 300, 1)):
        guards = GT.Guards()
        out5 = guards.host(5, np.int64, fill=-7)
        assert getattr(lib, GRID_PLAN)(ranges, queries, linear, C.c_void_p(out5.ctypes.data)) == 0
        guards.check()
        assert tuple(int(v) for v in out5) == _lib.bm25_grid_plan(ranges, queries, bool(linear))


# ---- the allocator itself ---------------------------------------------------------------------------------------------------------------
def test_the_host_guards_see_one_byte_on_either_side():
    for dtype, shape in ((np.int32, (3, 3)), (np.float64, 7), (np.int64, (0,)), (np.uint8, 5)):
        for at in (-1, None, -GT.MIN_GUARD, "far"):
            guards = GT.Guards()
            a = guards.host(shape, dtype, fill=0)
            assert (a.size == 0 or a.ctypes.data % 16 == a.itemsize % 16) and a.shape == (shape if isinstance(shape, tuple) else (shape,))
            assert guards.check() == 1
            _, buf, start, nbytes, _ = guards.made[0]
            assert start >= GT.MIN_GUARD and buf.shape[0] - start - nbytes >= max(GT.MIN_GUARD, nbytes)
            pos = start + nbytes if at is None else buf.shape[0] - 1 if at == "far" else start + at
            buf[pos] ^= 1
            with pytest.raises(AssertionError, match="guard bytes changed"):
                guards.check()


@gpu
def test_the_device_guards_see_one_byte_on_either_side(monkeypatch):
    import torch
    for dtype, shape in ((torch.int32, (3, 3)), (torch.float64, (7,)), (torch.int64, (129, 3))):
        for at in (-1, None):
            guards = GT.Guards()
            GT.patch_torch(monkeypatch, guards)
            t = torch.empty(shape, dtype=dtype, device="cuda")
            assert t.data_ptr() % 16 == t.element_size() and tuple(t.shape) == shape and len(guards.made) == 1
            t.zero_()
            assert guards.check() == 1
            _, buf, start, nbytes, _ = guards.made[0]
            assert start >= GT.MIN_GUARD and buf.shape[0] - start - nbytes >= max(GT.MIN_GUARD, nbytes)
            buf[start + nbytes if at is None else start + at] = 0
            with pytest.raises(AssertionError, match="guard bytes changed"):
                guards.check()
            monkeypatch.undo()


# ---- no entry is left out ------------------------------------------------------------------------------------------------------------
SCALARS = "its only outputs are scalar out-parameters"
STRUCT = "its only output is one struct"
EXEMPT = {
    "rag_comm_allgather_dev": "needs a communicator of several ranks; the two-rank tests run it",
    "rag_comm_unique_id": "the 128-byte id of a communicator, exchanged by the two-rank tests",
    "rag_comm_count": SCALARS,
    "rag_create": "its only output is the new handle",
    "rag_device_count": SCALARS, "rag_index_rows": SCALARS, "rag_index_insert_host": SCALARS, "rag_index_delete_host": SCALARS,
    "rag_index_deleted_rows": SCALARS, "rag_dense_kernel_ms": SCALARS, "rag_stage_kernel_ms": SCALARS, "rag_bm25_index_bytes": SCALARS,
    "rag_sparse_info": SCALARS, "rag_hybrid_linear_batch": SCALARS, "rag_tokens_info": SCALARS, "rag_embed_dim": SCALARS,
    "rag_tokvec_info": SCALARS, "rag_tokvec_form": SCALARS, "rag_ce_length_class": SCALARS, "rag_model_seq_limit": SCALARS,
    "rag_index_id_map_info": STRUCT, "rag_dense_last_stats": STRUCT, "rag_bm25_segment_stats": STRUCT, "rag_sparse_segment_stats": STRUCT,
}


def test_every_entry_that_writes_is_guarded_or_exempt():
    """(no GPU) The entries of include/rag_hip.h with a pointer to non-const other than the handle and `void* stream` = the entries
    the guarded cases name (each guarded run checks them against the entries it really called) + EXEMPT, and nothing else."""
    writes = GT.entries_that_write()
    declared = set(GT.header_declarations())
    assert len(writes) >= 100 and len([n for n in writes if n.endswith("_dev")]) >= 45
    named = {e for name in ENTRIES_A for e in ENTRIES_A[name]} | {e for name in R.CASES for e in R.ENTRIES[name]} | \
            {e for name in HOST_ENTRIES for e in HOST_ENTRIES[name]} | {GRID_PLAN}
    assert named <= declared, sorted(named - declared)
    assert set(EXEMPT) <= set(writes), sorted(set(EXEMPT) - set(writes))
    assert not named & set(EXEMPT), sorted(named & set(EXEMPT))
    assert (named & set(writes)) | set(EXEMPT) == set(writes), f"neither guarded nor exempt: {sorted(set(writes) - named - set(EXEMPT))}"
    assert all(isinstance(why, str) and len(why.split()) >= 4 for why in EXEMPT.values())
    # an entry with an array output never stands in EXEMPT: the binding types an array as void* and an out-parameter of one value as
    # a pointer to that value's type, so every writable parameter of an exempt entry (the communicator's three apart) is the latter
    from optimized_rag_amd import _lib
    one_value = type(C.POINTER(C.c_int))
    for name in sorted(set(EXEMPT) - {"rag_comm_allgather_dev", "rag_comm_unique_id", "rag_comm_count"}):
        params, sig = GT.header_declarations()[name][0], _lib._SIGS[name][0]
        assert len(params) == len(sig), name
        assert all(isinstance(t, one_value) for p, t in zip(params, sig) if p in writes[name]), (name, writes[name])
    assert set(RAGGED_A) <= set(ENTRIES_A) and set(RAGGED_R) <= set(R.CASES)
