"""GPU: the two row spaces of the MX classifier forward.

The MX forward of a classifier packs a pair's GEMM rows to a multiple of 4 (row_off) while attention keeps 16-row fragment tiles
(pair_off): a pair may start anywhere in a 128-row image tile, a 16-row attention tile may come from two image tiles, and the slots
of a pair's last attention tile past its rows rounded up to 4 are written by no GEMM. Every batch below is scored with option
ce_mx = 1 on the seeded MiniLM shape (6 layers, hidden 384, 12 heads, ffn 1536); each pair scored alone must give the bits it
gives in the batch, and the batch must give the bits recorded in tests/golden/ce_rows4_logits.npz from the build before the row
spaces were split (rows padded to 16 everywhere). The embedding model and the split-fp16 forward keep the granularity of 16 and are
pinned to their recorded bits as well."""
import os

import numpy as np
import pytest

from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

CFG = dict(vocab_size=2000, hidden=384, layers=6, heads=12, ffn=1536, max_pos=256, type_vocab=2, eps=1e-12)
SEED = 404
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ce_rows4_logits.npz")
POISON = 2                                        # the word-embedding row set to NaN; other tokens are drawn from [5, vocab)

# (a) 24 pairs at L = 64: every len % 16 of {0, 1, 3, 4, 5, 12, 13, 15}; rounded up to 4 the pair of 64 tokens starts at row 116 and
# the pair of 36 tokens at row 252, so rows 128 and 256 (image-tile boundaries) fall 12 and 4 rows into a pair
LENS_A = [17, 3, 16, 20, 5, 12, 13, 15, 1, 64, 33, 35, 36, 37, 44, 45, 47, 48, 19, 52, 21, 28, 61, 63]
# (b) 8 pairs at L = 128 and L = 256: lengths 1, 17 and L, and pairs with an odd count of 16-row tiles (40: 3, 77: 5; 200: 13, 37: 3)
LENS_B = {128: [1, 17, 128, 40, 77, 100, 5, 127], 256: [1, 17, 256, 200, 131, 250, 37, 99]}


def batch(lens, L, seed):
    lens = np.asarray(lens, dtype=np.int32)
    rng = np.random.default_rng(seed)
    ids = rng.integers(5, CFG["vocab_size"], (len(lens), L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 9) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return ids, tt, lens


def cases():
    """name -> (ids, tt, lens) of every recorded batch"""
    out = {"a": batch(LENS_A, 64, 1)}
    for L, lens in LENS_B.items():
        out[f"b{L}"] = batch(lens, L, L)
    return out


def tensors(w, head=True):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    return flatten_state_dict(w, CFG["layers"], head=head)


def with_mode(eng, mode, fn):
    eng.set_option("ce_mx", mode)
    try:
        return fn()
    finally:
        eng.set_option("ce_mx", 0)


def record(eng):
    """What the fixture holds, computed on `eng`: name -> array. `PYTHONPATH=. python tests/test_ce_row_spaces_gpu.py OUT.npz` (from the
    repository root) writes it with the library in use (RAG_HIP_LIB picks another build); the committed file came from the build before the change."""
    w = B.seeded_weights(CFG, SEED)
    out = {}
    eng.ce_load(CFG, tensors(w))
    for name, (ids, tt, lens) in cases().items():
        out[f"mx_{name}"] = with_mode(eng, 1, lambda: eng.ce_score(ids, tt, lens))
    ids, tt, lens = cases()["a"]
    out["split_a"] = with_mode(eng, -1, lambda: eng.ce_score(ids, tt, lens))
    eng.embed_load(CFG, tensors(w, head=False), normalize=True)
    out["embed_mx_a"] = with_mode(eng, 1, lambda: eng.embed(ids, tt, lens))
    out["embed_split_a"] = with_mode(eng, -1, lambda: eng.embed(ids, tt, lens))
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def weights():
    return B.seeded_weights(CFG, SEED)


@pytest.fixture(scope="module")
def eng(weights):
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=384, device=0)
    e.ce_load(CFG, tensors(weights))
    yield e
    e.close()


def _ceil(n, g):
    return (np.asarray(n) + g - 1) // g * g


def test_batch_a_crosses_two_image_tiles_off_the_16_row_grid():
    """The property of LENS_A the other tests rely on (host arithmetic only)."""
    assert {n % 16 for n in LENS_A} >= {0, 1, 3, 4, 5, 12, 13, 15} and len(LENS_A) == 24
    off = np.concatenate([[0], np.cumsum(_ceil(LENS_A, 4))])
    for edge in (128, 256):
        p = int(np.searchsorted(off, edge, side="right")) - 1
        assert off[p] < edge < off[p + 1] and (edge - off[p]) % 16 != 0 and off[p] % 16 != 0


def _alone_and_recorded(eng, golden, name):
    ids, tt, lens = cases()[name]
    got = with_mode(eng, 1, lambda: eng.ce_score(ids, tt, lens))
    assert np.isfinite(got).all()
    for i in range(len(lens)):
        alone = with_mode(eng, 1, lambda: eng.ce_score(ids[i:i + 1], tt[i:i + 1], lens[i:i + 1]))
        np.testing.assert_array_equal(alone, got[i:i + 1], err_msg=f"batch {name}: pair {i} (len {lens[i]}) alone")
    np.testing.assert_array_equal(got, golden[f"mx_{name}"], err_msg=f"batch {name} against the recorded logits")


def test_a_pairs_alone_in_the_batch_and_recorded(eng, golden):
    _alone_and_recorded(eng, golden, "a")


@pytest.mark.parametrize("L", sorted(LENS_B))
def test_b_longer_classes_alone_in_the_batch_and_recorded(eng, golden, L):
    _alone_and_recorded(eng, golden, f"b{L}")


def test_c_stale_slots_of_a_non_finite_forward_do_not_reach_the_next(weights):
    """First forward: 24 full-length pairs, all but the first holding a token whose word-embedding row is NaN, so the Q / K / V
    fragment tiles and the activation rows of the workspace are left non-finite. Second forward on the same handle: the lengths of
    batch (a), whose last attention tiles have slots no GEMM of this forward writes. Its logits are finite and the bits of the same
    call on a fresh handle."""
    from optimized_rag_amd import RagEngine
    w = {k: v.copy() for k, v in weights.items()}
    w["bert.embeddings.word_embeddings.weight"][POISON] = np.nan
    t = tensors(w)
    big_ids, big_tt, big_lens = batch([64] * 24, 64, 7)
    big_ids[1:, 5] = POISON
    ids, tt, lens = cases()["a"]
    used, fresh = RagEngine(dim=384, device=0), RagEngine(dim=384, device=0)
    try:
        used.ce_load(CFG, t)
        fresh.ce_load(CFG, t)
        big = with_mode(used, 1, lambda: used.ce_score(big_ids, big_tt, big_lens))
        assert np.isfinite(big[0]) and np.isnan(big[1:]).all()
        got = with_mode(used, 1, lambda: used.ce_score(ids, tt, lens))
        ref = with_mode(fresh, 1, lambda: fresh.ce_score(ids, tt, lens))
    finally:
        used.close()
        fresh.close()
    assert np.isfinite(got).all(), got
    np.testing.assert_array_equal(got, ref)


def test_d_embedding_model_and_split_forward_keep_their_bits(eng, weights, golden):
    ids, tt, lens = cases()["a"]
    np.testing.assert_array_equal(with_mode(eng, -1, lambda: eng.ce_score(ids, tt, lens)), golden["split_a"])
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=384, device=0)
    try:
        e.embed_load(CFG, tensors(weights, head=False), normalize=True)
        np.testing.assert_array_equal(with_mode(e, 1, lambda: e.embed(ids, tt, lens)), golden["embed_mx_a"])
        np.testing.assert_array_equal(with_mode(e, -1, lambda: e.embed(ids, tt, lens)), golden["embed_split_a"])
    finally:
        e.close()


if __name__ == "__main__":
    import sys
    from optimized_rag_amd import RagEngine
    _e = RagEngine(dim=384, device=0)
    try:
        np.savez(sys.argv[1], **record(_e))
    finally:
        _e.close()
