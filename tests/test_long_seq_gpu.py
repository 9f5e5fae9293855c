"""GPU: sequences past 512 tokens on models with 64-wide heads - the length classes 768 ... 8192, the streamed form of
ce_attention64_kernel (an LDS ring shared by the eight waves of a workgroup) and its DIRECT twin (option ce_attn_stream = -1) -
against the float64 oracle (oracle/bert_oracle.py, which takes max_pos from the config as it is). All models have 2 layers and
seeded weights; the default one is 128 / 2 (64-wide heads), ffn 512, vocab 2000, max_pos 8192.

Bars are the project's (tests/test_head64_gpu.py): logits within 4e-3, sigmoid scores within 1e-3, unit-vector components within 1e-3,
1 - cos < 1e-6, an un-normalised vector within 1e-3 * |exp|. Every test prints what it measured (pytest -s); the maxima measured on
an MI355X are in the docstrings and in DESIGN.md 4.5. The oracle runs each sequence alone at its own length (its result does not
depend on padding), once per sequence for all heads."""
import ctypes as C
import json

import numpy as np
import pytest

import xlmr_tools as X
from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

RAG_ERR_ARG, RAG_ERR_STATE = -1, -3
LOGIT_TOL = 4e-3
SCORE_TOL = 1e-3
EMB_TOL = 1e-3
COS_TOL = 1e-6
HEADS5 = ("classifier", "mean", "mean_raw", "cls", "cls_raw")


def _cfg(hidden, heads, ffn=None, vocab=2000, max_pos=8192):
    return dict(vocab_size=vocab, hidden=hidden, layers=2, heads=heads, ffn=ffn or 4 * hidden, max_pos=max_pos, type_vocab=2, eps=1e-12)


CFG = _cfg(128, 2)
SEED = 8192
_WEIGHTS = {}


def _weights(cfg, seed=SEED):
    key = (json.dumps(cfg, sort_keys=True), seed)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = B.seeded_weights(cfg, seed)
    return _WEIGHTS[key]


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=64, device=0)
    yield e
    e.close()


def _tensors(w, cfg, head=True):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    return flatten_state_dict(w, cfg["layers"], head=head)


def _load(eng, cfg, w, head):
    """Loads the model behind `head` and returns the call that runs it."""
    if head == "classifier":
        eng.ce_load(cfg, _tensors(w, cfg))
        return eng.ce_score
    eng.embed_load(cfg, _tensors(w, cfg, head=False), normalize=not head.endswith("_raw"), pooling=head.split("_")[0])
    return eng.embed


def _seqs(seed, cfg, lens, lo=5):
    """One token / type row per length (each as long as its sequence)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        ids = rng.integers(lo, cfg["vocab_size"], n).astype(np.int32)
        tt = (np.arange(n) >= 9).astype(np.int32)
        out.append((ids, tt))
    return out


def _batch(seqs, L):
    ids = np.zeros((len(seqs), L), dtype=np.int32)
    tt = np.zeros((len(seqs), L), dtype=np.int32)
    lens = np.array([len(s[0]) for s in seqs], dtype=np.int32)
    for i, (a, b) in enumerate(seqs):
        ids[i, :len(a)], tt[i, :len(a)] = a, b
    return ids, tt, lens


def _with_option(eng, name, value, fn):
    eng.set_option(name, value)
    try:
        return fn()
    finally:
        eng.set_option(name, 0)


def _oracle(cfg, w, seq):
    """Every head's float64 result for one sequence, from one pass of the encoder at the sequence's own length."""
    ids, tt = seq
    n = len(ids)
    W, x = B.forward_hidden(w, cfg, ids[None].astype(np.int64), tt[None].astype(np.int64), np.array([n]), fast_erf=True)
    x = x[0]
    pooled = np.tanh(x[0] @ W["bert.pooler.dense.weight"].T + W["bert.pooler.dense.bias"])
    unit = lambda v: v / max(np.linalg.norm(v), 1e-12)
    return {"classifier": (pooled @ W["classifier.weight"].T + W["classifier.bias"])[0], "mean": unit(x.mean(0)), "mean_raw": x.mean(0),
            "cls": unit(x[0]), "cls_raw": x[0]}


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


def _check(head, got, exp, what):
    """got against the oracle at the bars of the head; returns the measured figures."""
    assert np.isfinite(got).all(), what
    g, exp = got.astype(np.float64), np.asarray(exp)
    if head == "classifier":
        err, serr = np.abs(g - exp).max(), np.abs(_sigmoid(g) - _sigmoid(exp)).max()
        print(f"MEASURED {what} classifier: max |logit - oracle| = {err:.2e}, max |score - oracle| = {serr:.2e}")
        assert err < LOGIT_TOL and serr < SCORE_TOL, (what, err, serr)
    elif head.endswith("_raw"):
        rel = (np.abs(g - exp).max(1) / np.linalg.norm(exp, axis=1)).max()
        print(f"MEASURED {what} {head}: max |raw - oracle| / |oracle| = {rel:.2e}")
        assert rel < EMB_TOL, (what, head, rel)
    else:
        comp = np.abs(g - exp).max()
        cos = (1.0 - (g * exp).sum(1) / np.linalg.norm(g, axis=1)).max()
        print(f"MEASURED {what} {head}: max component error = {comp:.2e}, max 1 - cos = {cos:.2e}")
        assert comp < EMB_TOL and cos < COS_TOL, (what, head, comp, cos)


# ---- the calls of tests 1, 3 and 4: name -> (sequences, seq_len, ce_chunk_tokens). A result is computed once per (call, head, form).
P1025 = _seqs(11, CFG, [513, 544, 767, 768, 769, 1024, 1025, 1, 16, 300])
P513 = _seqs(12, CFG, [513, 40])
SHORT = _seqs(13, CFG, [5, 33, 200, 500])
NEIGHBOUR = _seqs(14, CFG, [700])
LONG = _seqs(15, CFG, [600, 1000])
CALLS = {
    "p1025": (P1025, 1025, 0),
    "p513": (P513, 513, 0),
    "short@512": (SHORT, 512, 0),
    "short@768": (NEIGHBOUR + SHORT, 768, 0),
    "short@4096": (NEIGHBOUR + SHORT, 4096, 0),
    "long@1024": (LONG, 1024, 0),
    "long@4096": (LONG, 4096, 0),
    "long@1024 in 3 chunks": (LONG + SHORT, 1024, 2 * 1024),          # 6 sequences, 2 per chunk
    "long@4096 in 3 chunks": (LONG + SHORT, 4096, 2 * 4096),
}
_RESULTS = {}
_LOADED = [None, None]


def _result(eng, call, head, form=0):
    """The float32 result of CALLS[call] on the default model's `head`, with option ce_attn_stream = form."""
    key = (call, head, form)
    if key not in _RESULTS:
        if _LOADED[0] != head:
            _LOADED[:] = [head, _load(eng, CFG, _weights(CFG), head)]
        seqs, L, chunk = CALLS[call]
        args = _batch(seqs, L)
        eng.set_option("ce_chunk_tokens", chunk)
        try:
            _RESULTS[key] = _with_option(eng, "ce_attn_stream", form, lambda: _LOADED[1](*args))
        finally:
            eng.set_option("ce_chunk_tokens", 0)
    return _RESULTS[key]


_ORACLE = {}


def _expected(name, seqs, head):
    if name not in _ORACLE:
        w = _weights(CFG)
        _ORACLE[name] = [_oracle(CFG, w, s) for s in seqs]
    return np.stack([o[head] for o in _ORACLE[name]])


# ---- 1. oracle parity across the boundary ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS5)
def test_oracle_parity_across_512(eng, head):
    """One call at seq_len 1025 (class 1536) with lengths 513, 544, 767, 768, 769, 1024, 1025, 1, 16, 300 - odd and even tile counts,
    exact class edges, short sequences beside long ones - and one at seq_len 513 (class 768) with 513 and 40, on every head. Before
    the long classes the first call returned RAG_ERR_ARG.
    Measured on an MI355X at seq_len 1025 / 513: logit 3.8e-6 / 1.8e-6, score 3.1e-8 / 4.7e-9; mean pooling component 3.1e-7 /
    1.7e-7, 1 - cos 2.1e-13 / 1.3e-13, raw 3.0e-7 / 1.6e-7; [CLS] pooling component 1.3e-7 / 1.0e-7, 1 - cos 1.0e-13 / 1.0e-13, raw
    1.3e-7 / 1.1e-7."""
    _check(head, _result(eng, "p1025", head), _expected("p1025", P1025, head), "seq_len 1025")
    _check(head, _result(eng, "p513", head), _expected("p513", P513, head), "seq_len 513")


# ---- 2. the top class -----------------------------------------------------------------------------------------------------------
def test_the_8192_class_matches_the_oracle(eng):
    """One call at seq_len 8192 with 8192, 4097 and 31 tokens: logits and mean-pooled unit vectors against the oracle.
    Measured on an MI355X: logit 1.4e-6, score 4.3e-9, component 4.7e-7, 1 - cos 7.7e-13."""
    seqs = _seqs(21, CFG, [8192, 4097, 31])
    w = _weights(CFG)
    exp = [_oracle(CFG, w, s) for s in seqs]
    args = _batch(seqs, 8192)
    for head in ("classifier", "mean"):
        _LOADED[:] = [head, _load(eng, CFG, w, head)]
        _check(head, _LOADED[1](*args), np.stack([o[head] for o in exp]), "seq_len 8192")


# ---- 3. invariance across the old limit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["classifier", "mean"])
def test_bits_do_not_depend_on_the_length_class_across_512(eng, head):
    """Sequences of 5, 33, 200 and 500 tokens scored at seq_len 512 (class 512: the kernels of before), then behind a 700-token
    sequence at seq_len 768 and 4096 (streamed attention): the same float32 bits. Sequences of 600 and 1000 tokens at seq_len 1024
    and 4096, and again in calls of six sequences that ce_chunk_tokens splits into three chunks: the same bits, and the short
    sequences riding in those calls still return their seq_len 512 bits. Against the oracle, measured on an MI355X: short sequences
    logit 1.2e-6, component 2.0e-7, 1 - cos 1.8e-13; 600 and 1000 tokens 3.0e-7, 1.8e-7, 1.8e-13."""
    short = _result(eng, "short@512", head)
    for call in ("short@768", "short@4096"):
        np.testing.assert_array_equal(_result(eng, call, head)[1:], short, err_msg=f"{head} {call}")
    np.testing.assert_array_equal(_result(eng, "short@768", head)[0], _result(eng, "short@4096", head)[0])
    long_ = _result(eng, "long@1024", head)
    np.testing.assert_array_equal(_result(eng, "long@4096", head), long_)
    for call in ("long@1024 in 3 chunks", "long@4096 in 3 chunks"):
        got = _result(eng, call, head)
        np.testing.assert_array_equal(got[:2], long_, err_msg=f"{head} {call}")
        np.testing.assert_array_equal(got[2:], short, err_msg=f"{head} {call}, the short sequences")
    _check(head, short, _expected("short", SHORT, head), "short sequences")
    _check(head, long_, _expected("long", LONG, head), "600 and 1000 tokens")


# ---- 4. streamed == DIRECT ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS5)
def test_the_streamed_form_returns_the_bits_of_the_direct_form(eng, head):
    """Every call of tests 1 and 3 again with option ce_attn_stream = -1 (DIRECT at every class above 256, its blockIdx.z grid
    extended to L / 256): bit-identical to the default."""
    calls = ("p1025", "p513") if head not in ("classifier", "mean") else tuple(CALLS)
    for call in calls:
        np.testing.assert_array_equal(_result(eng, call, head, -1), _result(eng, call, head, 0), err_msg=f"{head} {call}")


# ---- 5. other head counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,heads,lens", [(768, 12, [1100, 90]), (1024, 16, [530])], ids=["768/12", "1024/16"])
def test_other_head_counts_past_512(eng, hidden, heads, lens):
    """The BERT-base shape at seq_len 1100 (class 1536) and the BERT-large / XLM-R-large shape at 530 (class 768): logits and
    mean-pooled unit vectors against the oracle. Measured on an MI355X (logit / score / component / 1 - cos): 768/12 1.7e-4 / 1.2e-9 /
    5.4e-7 / 1.3e-11; 1024/16 1.2e-4 / 1.1e-5 / 3.5e-7 / 6.2e-12."""
    cfg = _cfg(hidden, heads, max_pos=1536)
    w = _weights(cfg, hidden)
    seqs = _seqs(hidden, cfg, lens)
    exp = [_oracle(cfg, w, s) for s in seqs]
    args = _batch(seqs, max(lens))
    _LOADED[:] = [None, None]
    for head in ("classifier", "mean"):
        _check(head, _load(eng, cfg, w, head)(*args), np.stack([o[head] for o in exp]), f"{hidden}/{heads} seq_len {max(lens)}")


# ---- 6. stale slack -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["classifier", "mean"])
def test_stale_rows_behind_an_odd_tile_count_are_not_read(head):
    """A call of 8 full 2048-token sequences fills the workspace; then, on the same handle, a call at seq_len 2048 whose last
    sequence has 513 tokens (33 tiles: tile 33 of its last 32-key block is slack that still holds the first call's K / V). It
    returns, bit for bit, what a freshly created handle returns for that call."""
    from optimized_rag_amd import RagEngine
    w = _weights(CFG)
    full = _batch(_seqs(61, CFG, [2048] * 8), 2048)
    second = _batch(_seqs(62, CFG, [2048, 100, 513]), 2048)
    used, fresh = RagEngine(dim=64, device=0), RagEngine(dim=64, device=0)
    try:
        run = _load(used, CFG, w, head)
        assert np.isfinite(run(*full)).all()
        got = run(*second)
        want = _load(fresh, CFG, w, head)(*second)
    finally:
        used.close()
        fresh.close()
    assert np.isfinite(want).all()
    np.testing.assert_array_equal(got, want)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def _limit(eng, which):
    out = C.c_int(-7)
    return eng.lib.rag_model_seq_limit(eng.h, which, C.byref(out)), out.value


def _refused(eng, entry, n_out, seq_len):
    """rag_ce_score_host / rag_embed_host on one all-zero sequence of seq_len tokens -> (return code, rag_last_error)."""
    ids = np.zeros((1, seq_len), dtype=np.int32)
    lens = np.array([seq_len], dtype=np.int32)
    out = np.zeros((1, n_out), dtype=np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = entry(eng.h, p(ids), p(ids), p(lens), 1, seq_len, p(out))
    return rc, eng.lib.rag_last_error(eng.h).decode()


def test_calls_past_the_models_limit_are_refused_and_the_handle_stays_usable():
    """32-wide heads with max_pos 8192 at seq_len 513; 64-wide heads at 8193; 64-wide heads with max_pos 600 at 601 (600 works):
    RAG_ERR_ARG with a message that names the limit and what set it, and a valid call afterwards matches the oracle.
    rag_model_seq_limit reports 512 / 8192 / 600, and RAG_ERR_STATE with nothing loaded. Measured on the calls after the refusals:
    logit at most 3.0e-6, component 1.7e-7, 1 - cos 1.3e-13."""
    from optimized_rag_amd import RagEngine, RagError
    e = RagEngine(dim=64, device=0)
    try:
        assert _limit(e, 0)[0] == RAG_ERR_STATE and _limit(e, 1)[0] == RAG_ERR_STATE
        assert _limit(e, 2)[0] == RAG_ERR_ARG and e.lib.rag_model_seq_limit(e.h, 0, None) == RAG_ERR_ARG
        with pytest.raises(RagError):
            e.model_seq_limit(0)
        narrow, wide, short = _cfg(128, 4), CFG, _cfg(128, 2, max_pos=600)
        for cfg, limit, word in ((narrow, 512, "head width"), (wide, 8192, "head width"), (short, 600, "max_position_embeddings")):
            w = _weights(cfg, 7)
            e.ce_load(cfg, _tensors(w, cfg))
            e.embed_load(cfg, _tensors(w, cfg, head=False))
            assert _limit(e, 0) == (0, limit) and _limit(e, 1) == (0, limit)
            assert e.model_seq_limit(0) == limit and e.model_seq_limit(1) == limit
            for entry, n_out in ((e.lib.rag_ce_score_host, 1), (e.lib.rag_embed_host, cfg["hidden"])):
                rc, msg = _refused(e, entry, n_out, limit + 1)
                assert rc == RAG_ERR_ARG and str(limit) in msg and word in msg, (limit, rc, msg)
            # the handle is still usable: a valid call right at the limit where that is cheap (600), a short one otherwise
            n = limit if limit == 600 else 300
            seqs = _seqs(limit, cfg, [n, 17])
            exp = [_oracle(cfg, w, s) for s in seqs]
            args = _batch(seqs, n)
            _check("classifier", e.ce_score(*args), np.stack([o["classifier"] for o in exp]), f"after the refusal at {limit + 1}")
            _check("mean", e.embed(*args), np.stack([o["mean"] for o in exp]), f"after the refusal at {limit + 1}")
        assert e.ce_length_class(64, 601) == 768 and e.ce_length_class(32, 512) == 512
        with pytest.raises(RagError):
            e.ce_length_class(32, 513)
    finally:
        e.close()


# ---- 8. through the Python classes ----------------------------------------------------------------------------------------------
WORDS = [f"w{i}" for i in range(60)]


def _xlmr_dir(tmp_path, name, head):
    hf = X.xlmr_hf_config(vocab_size=4000, hidden=128, heads=2, ffn=512, max_position_embeddings=2050)       # max_pos 2048
    sd = X.seeded_xlmr(hf, 81, head=head, prefix="roberta." if head else "")
    path = X.write_checkpoint(tmp_path / name, hf, sd, WORDS, np.linspace(4, 3999, len(WORDS)).astype(int))
    cfg = dict(vocab_size=4000, hidden=128, layers=2, heads=2, ffn=512, max_pos=2048, type_vocab=2, eps=1e-5)
    return path, cfg, X.xlmr_to_bert_names(sd, type_rows=2, head=head)


def _text(rng, n_words):
    return " ".join(rng.choice(WORDS, n_words))


def test_long_pairs_through_local_cross_encoder(tmp_path):
    """An XLM-R-style directory with 64-wide heads and max_pos 2048: LocalCrossEncoder.from_dir(max_length=1500).predict on pairs
    whose passages tokenise to more than 1000 tokens matches the oracle on the ids the tokenizer produced, and differs from the same
    pairs cut at max_length 512; with default arguments max_length stays 512. Measured on an MI355X: logit 4.2e-6, score 1.8e-8."""
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import LocalCrossEncoder
    path, cfg, bert = _xlmr_dir(tmp_path, "xlmr-long-ce", True)
    rng = np.random.default_rng(86)            # (seeds 82 .. 89 on the CPU, oracle alone: 86 moves both long logits by 2e-2 or more when cut)
    pairs = [(_text(rng, 12), _text(rng, 1100)), (_text(rng, 30), _text(rng, 1700)), (_text(rng, 5), _text(rng, 40))]
    e = RagEngine(dim=64, device=0)
    try:
        ce = LocalCrossEncoder.from_dir(path, max_length=1500, engine=e)
        assert ce.max_length == 1500 and e.model_seq_limit(0) == 2048
        ids, tt, lens = ce.tokenize_pairs(pairs)
        assert lens.tolist() == [1116, 1500, 49] and not tt.any()
        long_scores = ce.predict(pairs)
        assert LocalCrossEncoder.from_dir(path, max_length=5000, engine=e).max_length == 2048
        default = LocalCrossEncoder.from_dir(path, engine=e)
        assert default.max_length == 512 and default.tokenize_pairs(pairs)[2].tolist() == [512, 512, 49]
        cut_ids, cut_tt, cut_lens = default.tokenize_pairs(pairs)
        cut_scores = default.predict(pairs)
    finally:
        e.close()
    exp = np.array([_oracle(cfg, bert, (ids[i, :n], tt[i, :n]))["classifier"] for i, n in enumerate(lens)])
    _check("classifier", long_scores, exp, "LocalCrossEncoder max_length 1500")
    # the text cut at 512 tokens is another input: the oracle's two logits are further apart than both error bars together, so the
    # device's must differ; the short pair is the same input in both calls and returns the same bits
    cut_exp = np.array([_oracle(cfg, bert, (cut_ids[i, :n], cut_tt[i, :n]))["classifier"] for i, n in enumerate(cut_lens)])
    _check("classifier", cut_scores, cut_exp, "LocalCrossEncoder max_length 512")
    assert np.abs(exp[:2] - cut_exp[:2]).min() > 2 * LOGIT_TOL, (exp, cut_exp)
    assert (long_scores[:2] != cut_scores[:2]).all(), (long_scores, cut_scores)
    np.testing.assert_array_equal(long_scores[2], cut_scores[2])


def test_long_texts_through_local_embedding_service(tmp_path):
    """LocalEmbeddingService.from_dir(max_length=1500) gives the oracle's vector for a text of about 1200 tokens; with default
    arguments max_length stays 256. Measured on an MI355X: component 2.4e-7, 1 - cos 2.4e-13."""
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    path, cfg, bert = _xlmr_dir(tmp_path, "xlmr-long-enc", False)
    rng = np.random.default_rng(83)
    texts = [_text(rng, 1200), _text(rng, 20)]
    e = RagEngine(dim=128, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(path, max_length=1500, engine=e)
        assert svc.max_length == 1500 and e.model_seq_limit(1) == 2048
        ids, tt, lens = svc.tokenize(texts)
        assert lens.tolist() == [1202, 22]
        got = np.array(svc.generate_embeddings_batch(texts), dtype=np.float32)
        default = LocalEmbeddingService.from_dir(path, engine=e)
        assert default.max_length == 256 and default.tokenize(texts)[2].tolist() == [256, 22]
    finally:
        e.close()
    exp = np.stack([_oracle_encoder(cfg, bert, ids[i, :n]) for i, n in enumerate(lens)])
    _check("mean", got, exp, "LocalEmbeddingService max_length 1500")


def _oracle_encoder(cfg, w, ids):
    """The mean-pooled unit vector of an encoder without a pooler / classifier head."""
    return B.sentence_embeddings(w, cfg, ids[None].astype(np.int64), np.zeros((1, len(ids)), dtype=np.int64), np.array([len(ids)]),
                                 fast_erf=True)[0]
