"""GPU: the cross-encoder and embedding forwards at every shape ce_load accepts, pair independence under non-finite
activations, and the embedding model's multi-chunk loop, against the float64 oracle (oracle/bert_oracle.py). Bars as in
tests/test_cross_encoder_gpu.py: logits within 4e-3, sigmoid scores within 1e-3; unit embedding vectors within 1e-3 per component."""
import numpy as np
import pytest

from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

LOGIT_TOL = 4e-3
SCORE_TOL = 1e-3
EMB_TOL = 1e-3


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=384, device=0)
    yield e
    e.close()


def _tensors(w, cfg, head=True):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    return flatten_state_dict(w, cfg["layers"], head=head)


def _pairs(rng, cfg, lens, L, lo=5):
    ids = rng.integers(lo, cfg["vocab_size"], (len(lens), L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 9) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return ids, tt


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


def _with_mode(eng, mode, fn):
    eng.set_option("ce_mx", mode)
    try:
        return fn()
    finally:
        eng.set_option("ce_mx", 0)


def _check_both_heads(eng, cfg, seed, mode=0):
    """Classifier logits / scores and normalised embeddings of one model against the oracle on 5 of 12 pairs (lengths on the
    16-row edges)."""
    w = B.seeded_weights(cfg, seed)
    rng = np.random.default_rng(seed)
    L = 80
    lens = np.array([80, 1, 15, 16, 17, 31, 33, 48, 49, 64, 65, 79], dtype=np.int32)
    ids, tt = _pairs(rng, cfg, lens, L)
    sel = [0, 1, 5, 8, 11]
    i64 = lambda a: a[sel].astype(np.int64)
    eng.ce_load(cfg, _tensors(w, cfg))
    got = _with_mode(eng, mode, lambda: eng.ce_score(ids, tt, lens))
    exp = B.forward_logits(w, cfg, i64(ids), i64(tt), lens[sel], fast_erf=True)
    assert np.isfinite(got).all()
    err = np.abs(got[sel] - exp).max()
    assert err < LOGIT_TOL, (cfg, mode, err, got[sel], exp)
    assert np.abs(_sigmoid(got[sel]) - _sigmoid(exp)).max() < SCORE_TOL
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
    vec = _with_mode(eng, mode, lambda: eng.embed(ids, tt, lens))
    ref = B.sentence_embeddings(w, cfg, i64(ids), i64(tt), lens[sel], fast_erf=True)
    assert vec.shape == (len(lens), cfg["hidden"]) and np.isfinite(vec).all()
    assert np.abs(vec[sel] - ref).max() < EMB_TOL, (cfg, mode, np.abs(vec[sel] - ref).max())


@pytest.mark.parametrize("hidden,ffn", [(h, f) for h in range(128, 1025, 128) for f in (h, 4 * h)])
def test_every_loadable_hidden_size_scores_within_the_bar(eng, hidden, ffn):
    """Every hidden size ce_load accepts (multiples of 128 up to 1024, head dim 32), at FFN = hidden and 4 x hidden, 2 layers: the
    classifier and the embedding head on the default forward. Hidden 768 and 1024 are the 12- and 16-per-lane instances of the
    embedding / LayerNorm kernels with 24 and 32 heads; 640 and 896 (10 and 14 per lane) were accepted and then failed every call."""
    cfg = dict(vocab_size=2000, hidden=hidden, layers=2, heads=hidden // 32, ffn=ffn, max_pos=128, type_vocab=2, eps=1e-12)
    _check_both_heads(eng, cfg, hidden + ffn)


@pytest.mark.parametrize("ffn", [384, 768, 1152, 1536])
@pytest.mark.parametrize("mode", [1, -1], ids=["mx", "split16"])
def test_hidden_384_every_mx_ffn_width_on_both_forwards(eng, ffn, mode):
    """The MX forward takes hidden 384 with FFN 384, 768, 1152 or 1536 (1, 2, 3 or 4 feature tiles of the FFN-up GEMM, K = ffn for
    FFN-down): each on the MX and on the split-fp16 forward, classifier and embedding head."""
    cfg = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=ffn, max_pos=128, type_vocab=2, eps=1e-12)
    _check_both_heads(eng, cfg, 384 + ffn, mode)


@pytest.mark.parametrize("change", [dict(hidden=1152, heads=36), dict(hidden=192, heads=6), dict(heads=6), dict(ffn=200),
                                    dict(hidden=1280, heads=40, ffn=1280)])
def test_shapes_the_kernels_cannot_run_are_refused_at_load(eng, change):
    """A model the kernels cannot run is refused by ce_load / embed_load, not by every later call."""
    from optimized_rag_amd import RagError
    cfg = dict(vocab_size=100, hidden=384, layers=1, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    cfg.update(change)
    w = B.seeded_weights(cfg, 1)
    with pytest.raises(RagError, match="ce_load"):
        eng.ce_load(cfg, _tensors(w, cfg))
    with pytest.raises(RagError, match="ce_load"):
        eng.embed_load(cfg, _tensors(w, cfg, head=False))


# ---- pair independence: a pair with non-finite activations must not reach any other pair ------------------------------------
POISON = 2                                       # the word-embedding row set to NaN; other tokens are drawn from [5, vocab)
_NAN_CFG = dict(vocab_size=3000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=128, type_vocab=2, eps=1e-12)


def _nan_model():
    w = B.seeded_weights(_NAN_CFG, 31)
    w["bert.embeddings.word_embeddings.weight"][POISON] = np.nan
    return w


@pytest.mark.parametrize("mode", [0, 1, -1], ids=["default", "mx", "split16"])
def test_a_nan_pair_does_not_reach_the_pair_before_it(eng, mode):
    """Pairs A with an odd count of 16-row tiles (lengths 1-16 and 33-48: the second half of their last 32-key block lies in the
    next pair's rows), each followed by a pair B holding a token whose word-embedding row is NaN. Every A logit is finite,
    bit-identical to A scored alone, and within the bar of the oracle; the B logits are NaN."""
    cfg = _NAN_CFG
    w = _nan_model()
    eng.ce_load(cfg, _tensors(w, cfg))
    a_lens = [1, 7, 16, 33, 41, 48]
    lens = np.array([x for a in a_lens for x in (a, 40)], dtype=np.int32)
    rng = np.random.default_rng(4040)
    L = 64
    ids, tt = _pairs(rng, cfg, lens, L)
    ids[1::2, 3] = POISON
    got = _with_mode(eng, mode, lambda: eng.ce_score(ids, tt, lens))
    a = np.arange(0, len(lens), 2)
    assert np.isnan(got[1::2]).all()
    assert np.isfinite(got[a]).all(), got
    for i in a:
        alone = _with_mode(eng, mode, lambda: eng.ce_score(ids[i:i + 1], tt[i:i + 1], lens[i:i + 1]))
        np.testing.assert_array_equal(alone, got[i:i + 1])
    exp = B.forward_logits(w, cfg, ids[a].astype(np.int64), tt[a].astype(np.int64), lens[a], fast_erf=True)
    assert np.abs(got[a] - exp).max() < LOGIT_TOL


@pytest.mark.parametrize("mode", [0, 1, -1], ids=["default", "mx", "split16"])
def test_stale_nan_rows_of_a_larger_call_do_not_reach_a_later_call(eng, mode):
    """A 40-pair call whose pairs from the third on are poisoned leaves NaN activations in the workspace. A later 8-pair call (the
    same padded length: the workspace is reused) whose last pair has 3 tiles reads the 16 rows after its packed end, which the
    earlier call filled: its logits must be finite and bit-identical to the same call on a fresh handle."""
    from optimized_rag_amd import RagEngine
    cfg = _NAN_CFG
    w = _nan_model()
    tensors = _tensors(w, cfg)
    eng.ce_load(cfg, tensors)
    rng = np.random.default_rng(4141)
    L = 64
    big_lens = np.full(40, 64, dtype=np.int32)
    big_ids, big_tt = _pairs(rng, cfg, big_lens, L)
    big_ids[2:, 5] = POISON
    lens = np.array([64] * 7 + [40], dtype=np.int32)                 # packed end at row 7 * 64 + 48: inside poisoned pair 7
    ids, tt = _pairs(rng, cfg, lens, L)
    big = _with_mode(eng, mode, lambda: eng.ce_score(big_ids, big_tt, big_lens))
    assert np.isnan(big[2:]).all()
    got = _with_mode(eng, mode, lambda: eng.ce_score(ids, tt, lens))
    fresh = RagEngine(dim=384, device=0)
    try:
        fresh.ce_load(cfg, tensors)
        ref = _with_mode(fresh, mode, lambda: fresh.ce_score(ids, tt, lens))
    finally:
        fresh.close()
    assert np.isfinite(got).all(), got
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("mode", [0, 1, -1], ids=["default", "mx", "split16"])
def test_a_nan_text_does_not_reach_the_text_before_it(eng, mode):
    """The embedding twin of test_a_nan_pair_does_not_reach_the_pair_before_it. The mean pool reads every token row of its text, so it
    is the head that would show a neighbour's rows: texts A with an odd count of 16-row tiles, each followed by a poisoned text B,
    the last A at the packed end of a workspace that a fully poisoned 40-text call has just filled with NaN. Every A vector is
    finite, bit-identical to A embedded alone, and within the bar of the oracle; every component of the B vectors is NaN."""
    cfg = _NAN_CFG
    w = _nan_model()
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
    rng = np.random.default_rng(4242)
    L = 64
    big_lens = np.full(40, 64, dtype=np.int32)
    big_ids, big_tt = _pairs(rng, cfg, big_lens, L)
    big_ids[:, 5] = POISON
    a_lens = [1, 7, 16, 33, 41, 48]
    lens = np.array([x for a in a_lens for x in (a, 40)] + [33], dtype=np.int32)
    ids, tt = _pairs(rng, cfg, lens, L)
    tt[:] = 0
    ids[1::2, 3] = POISON
    big = _with_mode(eng, mode, lambda: eng.embed(big_ids, big_tt, big_lens))
    assert np.isnan(big).all()
    got = _with_mode(eng, mode, lambda: eng.embed(ids, tt, lens))
    a = np.arange(0, len(lens), 2)
    assert np.isnan(got[1::2]).all()
    assert np.isfinite(got[a]).all(), got[a]
    for i in a:
        alone = _with_mode(eng, mode, lambda: eng.embed(ids[i:i + 1], tt[i:i + 1], lens[i:i + 1]))
        np.testing.assert_array_equal(alone, got[i:i + 1])
    exp = B.sentence_embeddings(w, cfg, ids[a].astype(np.int64), tt[a].astype(np.int64), lens[a], fast_erf=True)
    assert np.abs(got[a] - exp).max() < EMB_TOL
    assert ((got[a] * exp).sum(1) > 1 - 1e-6).all()


# ---- lengths outside [1, seq_len] ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_in", [20, 32, 100])
@pytest.mark.parametrize("mode", [1, -1], ids=["mx", "split16"])
def test_out_of_range_lens_are_clamped_to_the_padded_length(eng, mode, l_in):
    """include/rag_hip.h: a length is clamped to [1, seq_len], seq_len being the caller's padded length and not the attention
    length class it is rounded up to (20 -> 32, 100 -> 128: tokens past seq_len do not exist, and a length of seq_len + 5 must not
    make the forward attend to, or pool over, padding). lens = 0, a negative one and seq_len + 5 give what the oracle gives at 1, 1
    and seq_len, on both heads; the row packing, the attention kernels and the mean pool read the one clamped value."""
    cfg = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=128, type_vocab=2, eps=1e-12)
    w = B.seeded_weights(cfg, 2718)
    rng = np.random.default_rng(l_in)
    given = np.array([0, l_in + 5, 12, -3, l_in + 5, l_in], dtype=np.int32)
    clamped = np.clip(given, 1, l_in)
    ids, tt = _pairs(rng, cfg, np.full(len(given), l_in, dtype=np.int32), l_in)         # real tokens in every position
    i64 = lambda x: x.astype(np.int64)
    eng.ce_load(cfg, _tensors(w, cfg))
    got = _with_mode(eng, mode, lambda: eng.ce_score(ids, tt, given))
    same = _with_mode(eng, mode, lambda: eng.ce_score(ids, tt, clamped))
    exp = B.forward_logits(w, cfg, i64(ids), i64(tt), clamped, fast_erf=True)
    assert np.isfinite(got).all()
    assert np.abs(got - exp).max() < LOGIT_TOL, (got, exp)
    assert np.abs(_sigmoid(got) - _sigmoid(exp)).max() < SCORE_TOL
    np.testing.assert_array_equal(got, same)
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
    vec = _with_mode(eng, mode, lambda: eng.embed(ids, tt, given))
    vsame = _with_mode(eng, mode, lambda: eng.embed(ids, tt, clamped))
    ref = B.sentence_embeddings(w, cfg, i64(ids), i64(tt), clamped, fast_erf=True)
    assert np.isfinite(vec).all()
    assert np.abs(vec - ref).max() < EMB_TOL
    assert ((vec * ref).sum(1) > 1 - 1e-6).all()
    np.testing.assert_array_equal(vec, vsame)


# ---- the embedding model's multi-chunk loop (out_width = hidden floats per pair) -----------------------------------------------
@pytest.mark.parametrize("l_in", [100, 300])
@pytest.mark.parametrize("hidden", [384, 128], ids=["h384-mx", "h128-split16"])
def test_embedding_multi_chunk_loop(eng, hidden, l_in):
    """Option ce_chunk_tokens = 4096 splits 300 texts into 10 chunks of 30 (L_in = 100, padded to 128) or 30 chunks of 10 (L_in =
    300, padded to 384): every chunk writes hidden floats per text at its own offset, through the host-pointer entry (staged per
    chunk) and the device-pointer entry. Both give the same bits as one chunk, and a sample matches the oracle."""
    import torch
    cfg = dict(vocab_size=3000, hidden=hidden, layers=2, heads=hidden // 32, ffn=4 * hidden, max_pos=512, type_vocab=2, eps=1e-12)
    w = B.seeded_weights(cfg, 17 + hidden)
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
    rng = np.random.default_rng(hidden + l_in)
    P = 300
    lens = rng.integers(1, l_in + 1, P).astype(np.int32)
    lens[[0, 9, 10, 29, 30, P - 1]] = [l_in, 16, 17, 33, l_in, 1]
    ids, tt = _pairs(rng, cfg, lens, l_in)
    one = eng.embed(ids, tt, lens)
    eng.set_option("ce_chunk_tokens", 4096)
    try:
        many = eng.embed(ids, tt, lens)
        dev = torch.empty((P, hidden), dtype=torch.float32, device="cuda")
        eng.embed_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(lens).cuda(), dev)
        torch.cuda.synchronize()
        dev = dev.cpu().numpy()
    finally:
        eng.set_option("ce_chunk_tokens", 0)
    assert np.isfinite(one).all()
    np.testing.assert_array_equal(many, one)
    np.testing.assert_array_equal(dev, one)
    sel = [0, 9, 10, 30, 151, P - 1]
    ref = B.sentence_embeddings(w, cfg, ids[sel].astype(np.int64), tt[sel].astype(np.int64), lens[sel], fast_erf=True)
    assert np.abs(one[sel] - ref).max() < EMB_TOL


# ---- the two forwards on one handle: their workspaces and their kernels' LDS limits are separate -----------------------------
_TWO_FWD_CFG = dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=512, type_vocab=2, eps=1e-12)


def _load_head(e, w, cfg, head):
    if head == "classifier":
        e.ce_load(cfg, _tensors(w, cfg))
    else:
        e.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)


def _run_head(e, head, mode, call):
    fn = e.ce_score if head == "classifier" else e.embed
    return _with_mode(e, mode, lambda: fn(*call))


def _first_call_of_a_fresh_handle(w, cfg, head, mode, call):
    from optimized_rag_amd import RagEngine
    fresh = RagEngine(dim=384, device=0)
    try:
        _load_head(fresh, w, cfg, head)
        return _run_head(fresh, head, mode, call)
    finally:
        fresh.close()


@pytest.mark.parametrize("head", ["classifier", "embedding"])
def test_workspaces_of_the_two_forwards_are_independent_across_resizes(eng, head):
    """One handle, alternating forwards: MX with 40 pairs at padded length 64, split-fp16 with 3 pairs at 32, MX with 8 pairs at 64
    (reuses the larger MX workspace; its last pair has 3 tiles, so its last 32-key block reaches into stale rows), the same split
    call again, MX with 5 pairs at 100 (reallocates to length class 128). Every result is bit-identical to the same call made as
    the first call of a fresh handle on that forward: neither forward resizes, evicts or dirties the other's buffers."""
    cfg = _TWO_FWD_CFG
    w = B.seeded_weights(cfg, 5150)
    rng = np.random.default_rng(5150)

    def call(lens, L):
        lens = np.asarray(lens, dtype=np.int32)
        return _pairs(rng, cfg, lens, L) + (lens,)

    mx40 = call(rng.integers(1, 65, 40), 64)
    sp3 = call([32, 5, 17], 32)
    mx8 = call([64] * 7 + [40], 64)
    mx5 = call([100, 1, 33, 64, 97], 100)
    steps = [(1, mx40), (-1, sp3), (1, mx8), (-1, sp3), (1, mx5)]
    _load_head(eng, w, cfg, head)
    got = [_run_head(eng, head, mode, c) for mode, c in steps]
    ref = {}
    for i, (mode, c) in enumerate(steps):
        if id(c) not in ref:
            ref[id(c)] = _first_call_of_a_fresh_handle(w, cfg, head, mode, c)
        assert np.isfinite(got[i]).all(), (i, got[i])
        np.testing.assert_array_equal(got[i], ref[id(c)], err_msg=f"step {i}")


def test_every_attention_instantiation_raises_its_own_lds_limit():
    """One pair of 300 tokens is length class 384: 96 KiB of dynamic LDS, the smallest class above the 64 KiB default, so each
    attention kernel instantiation must have had its own limit raised. One handle scores it on the split-fp16 and then on the MX
    forward, a second handle in the opposite order: both calls succeed on both, and the second call of each handle gives the
    bits of the other handle's first. Then 600 pairs at length 64 on the MX forward (the batched pooler, after the [CLS]-only
    attention launch was used): the first 3 logits are those of the same 3 pairs scored alone."""
    from optimized_rag_amd import RagEngine
    cfg = _TWO_FWD_CFG
    w = B.seeded_weights(cfg, 6160)
    rng = np.random.default_rng(6160)
    lens = np.array([300], dtype=np.int32)
    long_call = _pairs(rng, cfg, lens, 300) + (lens,)
    a, b = RagEngine(dim=384, device=0), RagEngine(dim=384, device=0)
    try:
        _load_head(a, w, cfg, "classifier")
        _load_head(b, w, cfg, "classifier")
        a_split = _run_head(a, "classifier", -1, long_call)
        a_mx = _run_head(a, "classifier", 1, long_call)
        b_mx = _run_head(b, "classifier", 1, long_call)
        b_split = _run_head(b, "classifier", -1, long_call)
        assert np.isfinite(a_split).all() and np.isfinite(b_mx).all()
        np.testing.assert_array_equal(a_mx, b_mx)
        np.testing.assert_array_equal(b_split, a_split)
        lens600 = rng.integers(1, 65, 600).astype(np.int32)
        ids600, tt600 = _pairs(rng, cfg, lens600, 64)
        many = _run_head(a, "classifier", 1, (ids600, tt600, lens600))
        alone = _run_head(a, "classifier", 1, (ids600[:3], tt600[:3], lens600[:3]))
        assert np.isfinite(many).all()
        np.testing.assert_array_equal(many[:3], alone)
    finally:
        a.close()
        b.close()
