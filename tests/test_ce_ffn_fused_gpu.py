"""GPU: the fused FFN launch of the MX forward (csrc/ce_mx.h mx_ffn_kernel) against the two launches it replaces.

Option ce_ffn_fused = 1 runs FFN-up and FFN-down of every layer tail as one persistent kernel whose intermediate lives in one slot
per workgroup, overwritten on every token tile; -1 runs FFN-up -> h8 -> FFN-down. Both forms do the same MFMAs in the same K
order, the same GELU and the same LayerNorm grouping, so every comparison here is bit for bit, on one handle, between the two
option values: seeded MiniLM-shape weights with 2 layers, option ce_mx = 1.

What can go wrong is the slot: a workgroup reads back what it stored a few K-steps earlier (a stale cache line or a store still in
flight would show), overwrites it on its next token tile (more than 256 x 128 packed rows: some workgroup takes a second tile), and
finds in it whatever an earlier chunk, call or batch left there. One feature tile (ffn 384) is a path of its own: FFN-down cannot be
prefetched under the only FFN-up tile, so the DMA stream restarts."""
import numpy as np
import pytest

from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

CFG = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=256, type_vocab=2, eps=1e-12)
SEED = 515
N_REUSE = 320                                     # pairs of the scratch-reuse batch
WORKGROUP_ROWS = 256 * 128                        # one token tile for each of 256 persistent workgroups


def batch(lens, L, seed, cfg=CFG):
    lens = np.asarray(lens, dtype=np.int32)
    rng = np.random.default_rng(seed)
    ids = rng.integers(5, cfg["vocab_size"], (len(lens), L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 9) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return ids, tt, lens


def reuse_lens():
    return np.random.default_rng(11).integers(4, 257, N_REUSE)


def tensors(w, cfg=CFG, head=True):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    return flatten_state_dict(w, cfg["layers"], head=head)


def with_fused(eng, mode, fn, **opts):
    """fn() with the MX forward forced, ce_ffn_fused = mode and the options in opts; every option back to 0 afterwards"""
    opts = dict(opts, ce_mx=1, ce_ffn_fused=mode)
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, 0)


def both(eng, fn, **opts):
    """fused, then two launches, then fused again on the same handle: all three the same bits"""
    fused = with_fused(eng, 1, fn, **opts)
    plain = with_fused(eng, -1, fn, **opts)
    assert np.isfinite(plain).all()
    np.testing.assert_array_equal(fused, plain)
    np.testing.assert_array_equal(with_fused(eng, 1, fn, **opts), plain)
    return plain


def engine(cfg=CFG, embed=False, **kw):
    from optimized_rag_amd import RagEngine
    w = B.seeded_weights(cfg, SEED)
    e = RagEngine(dim=384, device=0)
    if embed:
        e.embed_load(cfg, tensors(w, cfg, head=False), **kw)
    else:
        e.ce_load(cfg, tensors(w, cfg))
    return e


@pytest.fixture(scope="module")
def eng():
    e = engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def reuse_ref(eng):
    """the two-launch logits of the scratch-reuse batch in one chunk: computed once, compared against by several tests"""
    ids, tt, lens = batch(reuse_lens(), 256, 2)
    return with_fused(eng, -1, lambda: eng.ce_score(ids, tt, lens))


def test_one_token_tile(eng):
    """3 pairs = 8 + 36 + 128 packed rows: two token tiles, 254 workgroups without one (they leave before the first barrier)"""
    ids, tt, lens = batch([5, 33, 127], 128, 1)
    both(eng, lambda: eng.ce_score(ids, tt, lens))


def test_scratch_reuse(eng, reuse_ref):
    lens = reuse_lens()
    rows = int(((lens + 3) // 4 * 4).sum())
    assert rows > WORKGROUP_ROWS and rows % 128 != 0, rows          # a second tile into some slots, and a partial last tile
    ids, tt, lens = batch(lens, 256, 2)
    np.testing.assert_array_equal(both(eng, lambda: eng.ce_score(ids, tt, lens)), reuse_ref)


def test_stale_slots_between_batches_and_handles(eng, reuse_ref):
    """A, B, A on one handle (same lengths, other tokens), fused: B is B of a fresh handle, and A after B is A"""
    a = batch(reuse_lens(), 256, 2)
    b = batch(reuse_lens(), 256, 3)
    fresh = engine()
    try:
        b_fresh = with_fused(fresh, 1, lambda: fresh.ce_score(*b))
    finally:
        fresh.close()
    got = with_fused(eng, 1, lambda: [eng.ce_score(*a), eng.ce_score(*b), eng.ce_score(*a)])
    np.testing.assert_array_equal(got[0], reuse_ref)
    np.testing.assert_array_equal(got[1], b_fresh)
    np.testing.assert_array_equal(got[2], reuse_ref)
    assert not np.array_equal(got[0], got[1])
    np.testing.assert_array_equal(with_fused(eng, -1, lambda: eng.ce_score(*b)), b_fresh)


def test_several_chunks_per_call(eng, reuse_ref):
    ids, tt, lens = batch(reuse_lens(), 256, 2)
    chunk_tokens = 110 * 256                                        # 110 pairs of the class L = 256 per chunk: 3 chunks of 107, 107, 106
    assert -(-N_REUSE // (chunk_tokens // 256)) >= 3
    got = both(eng, lambda: eng.ce_score(ids, tt, lens), ce_chunk_tokens=chunk_tokens)
    np.testing.assert_array_equal(got, reuse_ref)


def test_classifier_cls_tail_in_one_tile(eng):
    """64 pairs: the last layer's tail runs on 64 compact [CLS] rows, half a token tile"""
    ids, tt, lens = batch(np.random.default_rng(5).integers(1, 65, 64), 64, 4)
    both(eng, lambda: eng.ce_score(ids, tt, lens))


@pytest.mark.parametrize("pooling", ["mean", "cls"])
def test_embedder_rows_in_sixteens(pooling):
    """the embedder keeps every layer on full rows padded to 16; both pooled outputs of embed()"""
    e = engine(embed=True, normalize=True, pooling=pooling)
    try:
        ids, tt, lens = batch(np.random.default_rng(6).integers(1, 129, 48), 128, 5)
        both(e, lambda: e.embed(ids, tt, lens))
    finally:
        e.close()


@pytest.mark.parametrize("ffn", [384, 768])
def test_narrow_ffn(ffn):
    """ffn 384: ONE up tile, FFN-down's stream restarts after its epilogue; ffn 768: two. 40 pairs over four token tiles"""
    cfg = dict(CFG, ffn=ffn)
    e = engine(cfg)
    try:
        ids, tt, lens = batch(np.random.default_rng(7).integers(1, 33, 40), 32, 6, cfg)
        both(e, lambda: e.ce_score(ids, tt, lens))
    finally:
        e.close()
