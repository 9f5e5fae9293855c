"""GPU: BERT models with 64-wide heads (BERT-base 768 / 12, BERT-large 1024 / 16, the small BERTs 128 / 2, 256 / 4, 512 / 8) on the
split-fp16 forward - the EPI_QKV64 epilogue and ce_attention64_kernel - and the [CLS] pooling mode of the embedding head, against the
float64 oracle (oracle/bert_oracle.py, pinned at head dim 64 by tests/test_head64_cpu.py). All models have 2 layers.

Bars are the project's (tests/test_cross_encoder_gpu.py, tests/test_embeddings_gpu.py): logits within 4e-3, sigmoid scores within
1e-3, unit-vector components within 1e-3, 1 - cos < 1e-6; an un-normalised vector within 1e-3 * |exp| per text.
Every test prints what it measured (pytest -s); the maxima measured on an MI355X are in the docstrings and in DESIGN.md 4.5."""
import ctypes as C
import json

import numpy as np
import pytest

from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

LOGIT_TOL = 4e-3
SCORE_TOL = 1e-3
EMB_TOL = 1e-3
COS_TOL = 1e-6


def _cfg(hidden, heads, ffn=None, vocab=2000, max_pos=128):
    return dict(vocab_size=vocab, hidden=hidden, layers=2, heads=heads, ffn=ffn or 4 * hidden, max_pos=max_pos, type_vocab=2, eps=1e-12)


BASE = _cfg(768, 12, max_pos=512)                 # the BERT-base shape
SMALL = _cfg(128, 2, max_pos=512)
MINILM = _cfg(384, 12, ffn=1536, max_pos=512)     # 32-wide heads: the MX forward's shape
_WEIGHTS = {}


def _weights(cfg, seed):
    key = (json.dumps(cfg, sort_keys=True), seed)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = B.seeded_weights(cfg, seed)
    return _WEIGHTS[key]


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=768, device=0)
    yield e
    e.close()


def _tensors(w, cfg, head=True):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    return flatten_state_dict(w, cfg["layers"], head=head)


def _pairs(rng, cfg, lens, L, lo=5):
    lens = np.asarray(lens, dtype=np.int32)
    ids = rng.integers(lo, cfg["vocab_size"], (len(lens), L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 9) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return ids, tt


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


def _i64(a):
    return np.asarray(a).astype(np.int64)


def _with_mode(eng, mode, fn):
    eng.set_option("ce_mx", mode)
    try:
        return fn()
    finally:
        eng.set_option("ce_mx", 0)


def _check_logits(got, exp, what):
    err, serr = np.abs(got - exp).max(), np.abs(_sigmoid(got) - _sigmoid(exp)).max()
    print(f"{what}: max |logit - oracle| = {err:.2e}, max |score - oracle| = {serr:.2e}")
    assert np.isfinite(got).all()
    assert err < LOGIT_TOL, (what, err)
    assert serr < SCORE_TOL, (what, serr)


def _check_unit(got, exp, what):
    g = got.astype(np.float64)
    comp = np.abs(g - exp).max()
    cos = (1.0 - (g * exp).sum(1) / np.linalg.norm(g, axis=1)).max()
    print(f"{what}: max component error = {comp:.2e}, max 1 - cos = {cos:.2e}")
    assert np.isfinite(got).all()
    assert comp < EMB_TOL, (what, comp)
    assert cos < COS_TOL, (what, cos)


def _check_raw(got, exp, what):
    rel = (np.abs(got.astype(np.float64) - exp).max(1) / np.linalg.norm(exp, axis=1)).max()
    print(f"{what}: max |raw - oracle| / |oracle| = {rel:.2e}")
    assert np.isfinite(got).all()
    assert rel < EMB_TOL, (what, rel)


def _both_heads(eng, cfg, w, ids, tt, lens, sel, what, mode=0):
    """Classifier logits / scores and normalised mean-pooled vectors of one model against the oracle on the rows `sel`."""
    exp_w, x = B.forward_hidden(w, cfg, _i64(ids[sel]), _i64(tt[sel]), lens[sel], fast_erf=True)
    pooled = np.tanh(x[:, 0] @ exp_w["bert.pooler.dense.weight"].T + exp_w["bert.pooler.dense.bias"])
    exp = (pooled @ exp_w["classifier.weight"].T + exp_w["classifier.bias"])[:, 0]
    ok = (np.arange(x.shape[1])[None, :] < lens[sel][:, None]).astype(np.float64)[:, :, None]
    ref = (x * ok).sum(1) / ok.sum(1)
    ref /= np.maximum(np.linalg.norm(ref, axis=1, keepdims=True), 1e-12)
    eng.ce_load(cfg, _tensors(w, cfg))
    got = _with_mode(eng, mode, lambda: eng.ce_score(ids, tt, lens))
    assert np.isfinite(got).all()
    _check_logits(got[sel], exp, what + " classifier")
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
    vec = _with_mode(eng, mode, lambda: eng.embed(ids, tt, lens))
    assert vec.shape == (len(lens), cfg["hidden"]) and np.isfinite(vec).all()
    _check_unit(vec[sel], ref, what + " embedding")
    return got, vec


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,heads,ffn", [(128, 2, 512), (256, 4, 1024), (512, 8, 2048), (768, 12, 3072), (1024, 16, 4096),
                                              (768, 12, 768)])
def test_every_head64_shape_scores_within_the_bar(eng, hidden, heads, ffn):
    """Both heads of every 64-wide-head shape at L = 80 with lengths on the 16-row edges, 5 of 12 pairs against the oracle (the
    d64 twin of test_every_loadable_hidden_size_scores_within_the_bar). Before 64-wide heads were supported the load raised.
    Measured on an MI355X (logit / score / component / 1 - cos): 128/2 2.5e-6 / 1.4e-7 / 2.3e-7 / 4.2e-13, 256/4 5.3e-6 / 1.2e-6 /
    2.4e-7 / 8.1e-13, 512/8 1.5e-5 / 1.5e-6 / 2.0e-7 / 7.7e-13, 768/12 9.8e-5 / 5.1e-6 / 2.8e-7 / 3.1e-12, 1024/16 1.2e-4 / 2.2e-7 /
    5.9e-7 / 1.4e-11, 768/12 with ffn 768 9.6e-5 / 2.3e-5 / 7.1e-7 / 1.5e-11."""
    cfg = _cfg(hidden, heads, ffn)
    w = _weights(cfg, hidden + ffn)
    rng = np.random.default_rng(hidden + ffn)
    lens = np.array([80, 1, 15, 16, 17, 31, 33, 48, 49, 64, 65, 79], dtype=np.int32)
    ids, tt = _pairs(rng, cfg, lens, 80)
    _both_heads(eng, cfg, w, ids, tt, lens, [0, 1, 5, 8, 11], f"{hidden}/{heads} ffn {ffn}")


# ---- 2. the length classes that do not fit in LDS ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seq_len", [300, 512])
def test_long_length_classes_match_the_oracle(eng, seq_len):
    """768 / 12 at seq_len 300 (class 384) and 512: the classes whose K / V planes exceed the LDS and are read from global memory
    in two workgroups per (head, pair). Lengths around 256 (the query split between the two workgroups), with odd and even tile
    counts; 4 of 8 pairs against the oracle, both heads. Measured (logit / score / component / 1 - cos): 300: 7.5e-5 / 3.7e-7 /
    3.6e-7 / 3.7e-12; 512: 1.7e-4 / 2.1e-7 / 6.0e-7 / 1.3e-11."""
    cfg = BASE
    w = _weights(cfg, 1300)
    rng = np.random.default_rng(seq_len)
    lens = np.array([1, 16, 255, 256, 257, 272, 273, seq_len], dtype=np.int32)
    ids, tt = _pairs(rng, cfg, lens, seq_len)
    _both_heads(eng, cfg, w, ids, tt, lens, [2, 4, 6, 7], f"768/12 seq_len {seq_len}")


# ---- 3. bit identity ----------------------------------------------------------------------------------------------------------------
SEQ_LENS = [1, 16, 17, 31, 32, 200]
L_INS = [32, 64, 128, 256, 384, 512]


def _pad(a, L):
    out = np.zeros((a.shape[0], L), dtype=np.int32)
    out[:, :a.shape[1]] = a
    return out


@pytest.mark.parametrize("head", ["classifier", "embedding"])
@pytest.mark.parametrize("model", ["768/12", "128/2"])
def test_bits_do_not_depend_on_length_class_neighbours_chunks_or_entry(eng, model, head):
    """Sequences of 1, 16, 17, 31, 32 and 200 tokens: each alone at its own length, then between two neighbours (one full-length, one
    with an odd tile count) in batches padded to 32, 64, 128, 256 (LDS-staged attention), 384 and 512 (global-memory attention);
    the 512 batch again with ce_chunk_tokens splitting it into chunks of 2 sequences; and through the device-pointer entry. Every
    result is the bits of the sequence alone, and the alone results are within the bars (measured: 768/12 logit 1.3e-4, component
    3.8e-7, 1 - cos 5.1e-12; 128/2 1.5e-6, 1.1e-7, 9.5e-14)."""
    import torch
    cfg = BASE if model == "768/12" else SMALL
    w = _weights(cfg, 77)
    if head == "classifier":
        eng.ce_load(cfg, _tensors(w, cfg))
        run = eng.ce_score
    else:
        eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
        run = eng.embed
    k = len(SEQ_LENS)
    ids, tt = _pairs(np.random.default_rng(515), cfg, SEQ_LENS, max(SEQ_LENS))
    lens = np.asarray(SEQ_LENS, dtype=np.int32)
    alone = np.stack([run(ids[i:i + 1, :n], tt[i:i + 1, :n], lens[i:i + 1])[0] for i, n in enumerate(SEQ_LENS)])
    if head == "classifier":
        _check_logits(alone, B.forward_logits(w, cfg, _i64(ids), _i64(tt), lens, fast_erf=True), f"{model} alone")
    else:
        _check_unit(alone, B.sentence_embeddings(w, cfg, _i64(ids), _i64(tt), lens, fast_erf=True), f"{model} alone")
    for L_in in L_INS:
        mine = [i for i, n in enumerate(SEQ_LENS) if n <= L_in]
        n_ids, n_tt = _pairs(np.random.default_rng(L_in), cfg, [L_in, max(1, (L_in // 2) | 1)], L_in)
        cut = min(L_in, ids.shape[1])
        b_ids = np.ascontiguousarray(np.concatenate([n_ids[:1], _pad(ids[mine, :cut], L_in), n_ids[1:]]))
        b_tt = np.ascontiguousarray(np.concatenate([n_tt[:1], _pad(tt[mine, :cut], L_in), n_tt[1:]]))
        b_lens = np.concatenate([[L_in], lens[mine], [max(1, (L_in // 2) | 1)]]).astype(np.int32)
        got = run(b_ids, b_tt, b_lens)
        np.testing.assert_array_equal(got[1:-1], alone[mine], err_msg=f"{model} {head} L_in={L_in}")
        if L_in in (64, 512):
            eng.set_option("ce_chunk_tokens", 2 * L_in)       # both are their own length class: 2 sequences per chunk
            try:
                chunked = run(b_ids, b_tt, b_lens)
                out = torch.empty(got.shape, dtype=torch.float32, device="cuda")
                dev_args = [torch.from_numpy(a).cuda() for a in (b_ids, b_tt, b_lens)]
                (eng.ce_score_dev if head == "classifier" else eng.embed_dev)(*dev_args, out)
                torch.cuda.synchronize()
                chunked_dev = out.cpu().numpy()
            finally:
                eng.set_option("ce_chunk_tokens", 0)
            np.testing.assert_array_equal(chunked, got, err_msg=f"{model} {head} L_in={L_in} chunked")
            np.testing.assert_array_equal(chunked_dev, got, err_msg=f"{model} {head} L_in={L_in} chunked, device entry")
            out = torch.empty(got.shape, dtype=torch.float32, device="cuda")
            (eng.ce_score_dev if head == "classifier" else eng.embed_dev)(*dev_args, out)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.cpu().numpy(), got, err_msg=f"{model} {head} L_in={L_in} device entry")


# ---- 4. pair independence: a pair with non-finite activations must not reach any other pair ------------------------------------
POISON = 2                                       # the word-embedding row set to NaN; other tokens are drawn from [5, vocab)
NAN_CFG = _cfg(768, 12, vocab=3000, max_pos=512)


def _nan_model():
    key = "nan"
    if key not in _WEIGHTS:
        w = dict(B.seeded_weights(NAN_CFG, 31))
        w["bert.embeddings.word_embeddings.weight"] = w["bert.embeddings.word_embeddings.weight"].copy()
        w["bert.embeddings.word_embeddings.weight"][POISON] = np.nan
        _WEIGHTS[key] = w
    return _WEIGHTS[key]


def _a_pairs_between_poisoned_pairs(eng, head, a_lens, b_len, L, seed):
    """Pairs A (odd counts of 16-row tiles: the second half of their last 32-key block lies in the next pair's rows), each followed
    by a poisoned pair B. Every A result is finite, the bits of A alone, and within the bar; every B result is NaN. Measured on the A
    pairs: logit 6.0e-5 at L = 64, 6.6e-5 at L = 304; component 3.0e-7, 1 - cos 3.2e-12 at L = 304."""
    cfg, w = NAN_CFG, _nan_model()
    if head == "classifier":
        eng.ce_load(cfg, _tensors(w, cfg))
        run = eng.ce_score
    else:
        eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
        run = eng.embed
    lens = np.array([x for a in a_lens for x in (a, b_len)], dtype=np.int32)
    ids, tt = _pairs(np.random.default_rng(seed), cfg, lens, L)
    ids[1::2, 3] = POISON
    got = run(ids, tt, lens)
    a = np.arange(0, len(lens), 2)
    assert np.isnan(got[1::2]).all()
    assert np.isfinite(got[a]).all(), got[a]
    for i in a:
        np.testing.assert_array_equal(run(ids[i:i + 1], tt[i:i + 1], lens[i:i + 1]), got[i:i + 1])
    if head == "classifier":
        _check_logits(got[a], B.forward_logits(w, cfg, _i64(ids[a]), _i64(tt[a]), lens[a], fast_erf=True), f"A pairs, L = {L}")
    else:
        _check_unit(got[a], B.sentence_embeddings(w, cfg, _i64(ids[a]), _i64(tt[a]), lens[a], fast_erf=True), f"A texts, L = {L}")


def test_a_nan_pair_does_not_reach_the_pair_before_it(eng):
    _a_pairs_between_poisoned_pairs(eng, "classifier", [1, 7, 16, 33, 41, 48], 40, 64, 4040)


def test_a_nan_text_does_not_reach_the_text_before_it(eng):
    """The embedding twin, after a fully poisoned 40-text call has filled the workspace with NaN (the last A text sits at the packed
    end: its last key block reaches into those stale rows). Measured on the A texts: component 5.5e-7, 1 - cos 1.1e-11."""
    cfg, w = NAN_CFG, _nan_model()
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
    rng = np.random.default_rng(4242)
    L = 64
    big_lens = np.full(40, 64, dtype=np.int32)
    big_ids, big_tt = _pairs(rng, cfg, big_lens, L)
    big_ids[:, 5] = POISON
    lens = np.array([x for a in [1, 7, 16, 33, 41, 48] for x in (a, 40)] + [33], dtype=np.int32)
    ids, tt = _pairs(rng, cfg, lens, L)
    ids[1::2, 3] = POISON
    assert np.isnan(eng.embed(big_ids, big_tt, big_lens)).all()
    got = eng.embed(ids, tt, lens)
    a = np.arange(0, len(lens), 2)
    assert np.isnan(got[1::2]).all()
    assert np.isfinite(got[a]).all(), got[a]
    for i in a:
        np.testing.assert_array_equal(eng.embed(ids[i:i + 1], tt[i:i + 1], lens[i:i + 1]), got[i:i + 1])
    _check_unit(got[a], B.sentence_embeddings(w, cfg, _i64(ids[a]), _i64(tt[a]), lens[a], fast_erf=True), "A texts after a NaN call")


def test_stale_nan_rows_of_a_larger_call_do_not_reach_a_later_call(eng):
    """A 40-pair call poisoned from the third pair on leaves NaN in the workspace; a later 8-pair call of the same padded length whose
    last pair has 3 tiles reads the 16 rows after its packed end. Its logits are finite and the bits of a fresh handle's."""
    from optimized_rag_amd import RagEngine
    cfg, w = NAN_CFG, _nan_model()
    tensors = _tensors(w, cfg)
    eng.ce_load(cfg, tensors)
    rng = np.random.default_rng(4141)
    L = 64
    big_lens = np.full(40, 64, dtype=np.int32)
    big_ids, big_tt = _pairs(rng, cfg, big_lens, L)
    big_ids[2:, 5] = POISON
    lens = np.array([64] * 7 + [40], dtype=np.int32)
    ids, tt = _pairs(rng, cfg, lens, L)
    assert np.isnan(eng.ce_score(big_ids, big_tt, big_lens)[2:]).all()
    got = eng.ce_score(ids, tt, lens)
    fresh = RagEngine(dim=768, device=0)
    try:
        fresh.ce_load(cfg, tensors)
        ref = fresh.ce_score(ids, tt, lens)
    finally:
        fresh.close()
    assert np.isfinite(got).all(), got
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("head", ["classifier", "embedding"])
def test_a_nan_pair_does_not_reach_the_pair_before_it_above_256_tokens(eng, head):
    """Length class 384 (the global-memory attention): A pairs of 17 and 19 tiles, whose last key block's second half is the first
    tile of the poisoned pair behind them - the instance selects zeros for V there instead of reading it."""
    _a_pairs_between_poisoned_pairs(eng, head, [257, 272, 289, 300], 300, 304, 4343)


# ---- 5. lengths outside [1, seq_len] -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_in", [20, 300])
def test_out_of_range_lens_are_clamped_to_the_padded_length(eng, l_in):
    """lens = 0, a negative one and seq_len + 5 give what the oracle gives at 1, 1 and seq_len, on both heads of a 768 / 12 model, in
    a staged (20 -> 32) and a global-memory (300 -> 384) length class; and the bits of the call with the clamped lengths. Measured
    (logit / component / 1 - cos): 20: 1.8e-5 / 1.9e-7 / 1.0e-12; 300: 8.8e-5 / 3.4e-7 / 2.7e-12."""
    cfg = BASE
    w = _weights(cfg, 2718)
    rng = np.random.default_rng(l_in)
    given = np.array([0, l_in + 5, 12, -3, l_in + 5, l_in], dtype=np.int32)
    clamped = np.clip(given, 1, l_in)
    ids, tt = _pairs(rng, cfg, np.full(len(given), l_in, dtype=np.int32), l_in)         # real tokens in every position
    sel = [0, 1, 3]
    eng.ce_load(cfg, _tensors(w, cfg))
    got, same = eng.ce_score(ids, tt, given), eng.ce_score(ids, tt, clamped)
    np.testing.assert_array_equal(got, same)
    _check_logits(got[sel], B.forward_logits(w, cfg, _i64(ids[sel]), _i64(tt[sel]), clamped[sel], fast_erf=True), f"clamped, L_in {l_in}")
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=True)
    vec, vsame = eng.embed(ids, tt, given), eng.embed(ids, tt, clamped)
    np.testing.assert_array_equal(vec, vsame)
    _check_unit(vec[sel], B.sentence_embeddings(w, cfg, _i64(ids[sel]), _i64(tt[sel]), clamped[sel], fast_erf=True), f"clamped, L_in {l_in}")


# ---- 6. stress weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["sharp", "combined"])
def test_stress_weights_stay_within_the_bars(eng, level):
    """tests/ce_stress.py's sharp(2) (attention logits x 4: where a 64-term score sum is most exposed) and combined (sharp(1.5) +
    outliers(8) + ffn_tails(3)) transforms of a 768 / 12 model, both heads, 5 of 10 pairs at L = 128. Measured (logit / score /
    component / 1 - cos): sharp 2.0e-4 / 2.2e-7 / 4.7e-7 / 8.3e-12; combined 3.9e-5 / 5.3e-6 / 2.0e-6 / 5.9e-12."""
    import ce_stress as S
    cfg = _cfg(768, 12, vocab=3000, max_pos=128)
    w = _weights(cfg, 99)
    w = S.sharp(w, cfg, 2) if level == "sharp" else S.ffn_tails(S.outliers(S.sharp(w, cfg, 1.5), cfg, 8), cfg, 3)
    lens = np.array([128, 1, 15, 16, 17, 31, 33, 64, 65, 127], dtype=np.int32)
    ids, tt = _pairs(np.random.default_rng(2468), cfg, lens, 128, lo=1000)
    _both_heads(eng, cfg, w, ids, tt, lens, [0, 1, 4, 6, 9], f"768/12 {level}")


# ---- 7. refusals, and the 32-wide shapes beside a 64-wide model -------------------------------------------------------------------
@pytest.mark.parametrize("hidden,heads", [(256, 16), (1024, 8), (384, 6)])
def test_other_head_dims_are_refused_at_load(eng, hidden, heads):
    """Head dims 16 and 128 are refused by ce_load and embed_load with a ce_load message; so is 64 at hidden 384, the MX forward's
    width."""
    from optimized_rag_amd import RagError
    cfg = dict(vocab_size=100, hidden=hidden, layers=1, heads=heads, ffn=hidden, max_pos=64, type_vocab=2, eps=1e-12)
    w = B.seeded_weights(cfg, 1)
    with pytest.raises(RagError, match="ce_load"):
        eng.ce_load(cfg, _tensors(w, cfg))
    with pytest.raises(RagError, match="ce_load"):
        eng.embed_load(cfg, _tensors(w, cfg, head=False))


def test_a_32_wide_model_scores_the_same_bits_before_and_after_a_64_wide_one(eng):
    """A 384 / 12 model on the split-fp16 forward (ce_mx = -1), at a staged and at a long length class: scored, then a 768 / 12
    embedder is loaded beside it and run, then a 768 / 12 classifier replaces it and runs, then the 384 / 12 model is loaded again.
    Its logits are the same bits every time: the two head dims share the workspace type, the GEMM's LDS attribute and the handle."""
    cfg, w = MINILM, _weights(MINILM, 5150)
    w64 = _weights(BASE, 77)
    rng = np.random.default_rng(5150)
    calls = []
    for L in (80, 300):
        lens = np.array([L, 1, 17, 33, L - 1], dtype=np.int32)
        calls.append(_pairs(rng, cfg, lens, L) + (lens,))
    score = lambda: [_with_mode(eng, -1, lambda: eng.ce_score(*c)) for c in calls]
    eng.ce_load(cfg, _tensors(w, cfg))
    first = score()
    _check_logits(first[0], B.forward_logits(w, cfg, _i64(calls[0][0]), _i64(calls[0][1]), calls[0][2], fast_erf=True), "384/12 split16")
    eng.embed_load(BASE, _tensors(w64, BASE, head=False), normalize=True)
    assert all(np.isfinite(eng.embed(*c)).all() for c in calls)
    for a, b in zip(first, score()):
        np.testing.assert_array_equal(a, b)
    eng.ce_load(BASE, _tensors(w64, BASE))
    assert all(np.isfinite(eng.ce_score(*c)).all() for c in calls)
    eng.ce_load(cfg, _tensors(w, cfg))
    for a, b in zip(first, score()):
        np.testing.assert_array_equal(a, b)


# ---- 8. [CLS] pooling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,mode", [("384/12", 1), ("384/12", -1), ("768/12", 0)], ids=["384-mx", "384-split16", "768-head64"])
def test_cls_pooling_matches_the_first_row_of_the_oracle(eng, model, mode):
    """embed_load(..., pooling="cls"): the last hidden state of row 0, no pooler dense or tanh, with and without normalisation,
    against forward_hidden(...)[1][:, 0]; on both instantiations of the pooling kernel (MX and split fp16). The mean-pooled vectors
    of the same model differ from it: the flag is not ignored. Before the pooling mode existed, `pooling` was an unknown argument.
    Measured (component / 1 - cos / raw error over |exp|): 384/12 MX 1.4e-5 / 2.3e-9 / 1.4e-5; 384/12 split fp16 3.1e-7 / 8.6e-13 /
    3.1e-7; 768/12 3.5e-6 / 4.5e-10 / 3.5e-6."""
    cfg = MINILM if model == "384/12" else BASE
    w = _weights(cfg, 808)
    lens = np.array([80, 1, 15, 16, 17, 33, 64, 79], dtype=np.int32)
    ids, tt = _pairs(np.random.default_rng(808), cfg, lens, 80)
    tt[:] = 0
    _, x = B.forward_hidden(w, cfg, _i64(ids), _i64(tt), lens, fast_erf=True)
    raw = x[:, 0]
    unit = raw / np.maximum(np.linalg.norm(raw, axis=1, keepdims=True), 1e-12)
    t = _tensors(w, cfg, head=False)
    eng.embed_load(cfg, t, normalize=True, pooling="cls")
    got = _with_mode(eng, mode, lambda: eng.embed(ids, tt, lens))
    _check_unit(got, unit, f"{model} mode {mode} cls, normalised")
    eng.embed_load(cfg, t, normalize=False, pooling="cls")
    got_raw = _with_mode(eng, mode, lambda: eng.embed(ids, tt, lens))
    _check_raw(got_raw, raw, f"{model} mode {mode} cls, raw")
    eng.embed_load(cfg, t, normalize=True, pooling="mean")
    mean = _with_mode(eng, mode, lambda: eng.embed(ids, tt, lens))
    assert np.abs(mean[0] - got[0]).max() > 1e-2                     # an 80-token text: its mean is not its [CLS] row
    np.testing.assert_array_equal(mean[1], got[1])                   # a 1-token text: the mean over one row IS that row


@pytest.mark.parametrize("flags", [4, 7, 8, -1])
def test_unknown_flag_bits_of_embed_load_are_refused(eng, flags):
    from optimized_rag_amd import RagError
    from optimized_rag_amd._lib import CeConfig, _P
    cfg = _cfg(128, 2, max_pos=64, vocab=100)
    arrs = _tensors(B.seeded_weights(cfg, 1), cfg, head=False)
    c = CeConfig(cfg["vocab_size"], cfg["hidden"], cfg["layers"], cfg["heads"], cfg["ffn"], cfg["max_pos"], 2, 0, 1e-12)
    ptrs = (_P * len(arrs))(*[a.ctypes.data for a in arrs])
    with pytest.raises(RagError):
        eng._check(eng.lib.rag_embed_load_host(eng.h, C.byref(c), ptrs, len(arrs), flags), "rag_embed_load_host")
    for ok in (0, 1, 2, 3):
        eng._check(eng.lib.rag_embed_load_host(eng.h, C.byref(c), ptrs, len(arrs), ok), "rag_embed_load_host")


# ---- a BERT-base-shaped [CLS] checkpoint through the mirror classes -------------------------------------------------------------
def test_cls_pooled_bert_base_checkpoint_feeds_a_768_wide_index(tmp_path):
    """LocalEmbeddingService.from_dir on a generated 768 / 12 checkpoint directory whose 1_Pooling/config.json says [CLS]: vectors of
    dimension 768 that match the oracle's [CLS] rows (measured: component 1.2e-6, 1 - cos 4.6e-11), a GpuDocumentIndex of dim 768
    built from them, and search() finds each text."""
    from safetensors.numpy import save_file
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.document_store import GpuDocumentIndex
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    cfg = _cfg(768, 12, vocab=200, max_pos=64)
    w = _weights(cfg, 5)
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(195)]
    d = tmp_path / "bert-base-cls"
    (d / "1_Pooling").mkdir(parents=True)
    (d / "vocab.txt").write_text("\n".join(words) + "\n")
    (d / "config.json").write_text(json.dumps(dict(vocab_size=200, hidden_size=768, num_hidden_layers=2, num_attention_heads=12,
                                                   intermediate_size=3072, max_position_embeddings=64, type_vocab_size=2,
                                                   hidden_act="gelu", layer_norm_eps=1e-12)))
    (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(word_embedding_dimension=768, pooling_mode_cls_token=True,
                                                                 pooling_mode_mean_tokens=False, pooling_mode_max_tokens=False,
                                                                 pooling_mode_mean_sqrt_len_tokens=False)))
    save_file({k[len("bert."):]: v for k, v in w.items() if k.startswith("bert.") and "pooler" not in k}, str(d / "model.safetensors"))
    e = RagEngine(dim=768, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(str(d), engine=e)
        assert svc.pooling == "cls" and svc.get_embedding_dimension() == 768
        rng = np.random.default_rng(1)
        texts = list(dict.fromkeys(" ".join(rng.choice(words[5:], int(rng.integers(3, 40)))) for _ in range(60)))
        vecs = np.asarray(svc.generate_embeddings_batch(texts), dtype=np.float32)
        assert vecs.shape == (len(texts), 768)
        np.testing.assert_array_equal(np.asarray(svc.generate_embedding(texts[7], use_cache=False), dtype=np.float32), vecs[7])
        ids, tt, lens = svc.tokenize(texts[:4])
        raw = B.forward_hidden(w, cfg, _i64(ids), _i64(tt), lens, fast_erf=True)[1][:, 0]
        _check_unit(vecs[:4], raw / np.linalg.norm(raw, axis=1, keepdims=True), "from_dir, cls")
        idx = GpuDocumentIndex(svc, dim=768, engine=e)
        idx.bulk_load([{"content": t, "agent_id": "a"} for t in texts], vecs)
        for t in texts[:10]:
            hit = idx.search("a", t, top_k=1, with_embeddings=False)
            assert len(hit) == 1 and hit[0]["content"] == t and hit[0]["score"] > 1 - 1e-6
    finally:
        e.close()
